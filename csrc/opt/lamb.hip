// LAMB (You et al. 2020) and AdamW over ONE flat fp32 parameter buffer, on the segment / chunk table of
// lars.hip (one segment per parameter tensor, chunks of at most kLambChunk elements).  Per segment, at
// update number t = done + 1 with bc1 = 1 - beta1^t and bc2 = 1 - beta2^t (float64, rounded to fp32):
//   m = beta1 m + (1 - beta1) g ;  v = beta2 v + (1 - beta2) g g
//   u = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps) + wd_eff p          (wd_eff = excluded ? 0 : wd)
//   trust = excluded or |p| == 0 or |u| == 0 ? 1 : float(|p| / |u|)  (float64 sums of squares)
//   p -= lr trust u
// The direction u depends on the moments this step writes, so unlike LARS the norm pass is not a
// read-only pass:
//   moments : one block per chunk; loads p, g, m, v, stores m, v, writes (sum p^2, sum u^2) in
//             float64 to partials[chunk].  A chunk of an excluded segment has trust 1 by
//             construction and is finished here (p and the bf16 mirror written);
//   trust   : one wave per segment sums its chunks' partials and writes trust[seg]; its first block
//             also writes the bias corrections into the device record and advances the counter;
//   update  : one block per chunk of the open segments; re-reads p, m, v, recomputes u (the bytes of
//             a stashed u, and no buffer for it), p -= lr trust u and the mirror.
// With trust off (AdamW) one instantiation of the first pass updates every chunk, and a one-thread
// launch advances the counter: a launch never both reads the counter and advances it.
// No floating-point atomics; the sum of a chunk (per-thread order, wave butterfly, 4 waves) and of a
// segment (lane k takes chunks k, k+64, ..., then the butterfly) are fixed by the table alone, so
// the grid, the stream and the segment range of a launch never change a bit of the result.
// Gradient-norm clipping (clip.hip): with a clip record the first pass multiplies every gradient
// element by the record's coefficient as it loads it (one fp32 rounding, what an in-place scale pass
// would have stored); the gradient buffer itself stays unscaled.  trust_clip clamps the ratio at 1.
#include "kernels/common.h"
#include "opt/clip.h"
#include "opt/lamb.h"

#include <algorithm>
#include <stdexcept>

namespace pdt::opt {

constexpr uint32_t kExcludedBit = 0x80000000u;  // LarsChunk::seg bit 31 = the segment's flag bit 0

struct Table {
  const LarsSeg* segs;
  const LarsChunk* chunks;
  int nseg, nchunks;
  int64_t numel;
};

// fp32 coefficients of the element math
struct Coef {
  float b1, omb1, b2, omb2, eps, wd, nlr;  // nlr = -lr
};

// chunk range of the segments [seg_lo, seg_hi) (the launchers checked 0 <= seg_lo < seg_hi <= nseg)
__device__ __forceinline__ void chunk_range(const Table& t, int seg_lo, int seg_hi, int& c0, int& c1) {
  c0 = max(t.segs[seg_lo].chunk0, 0);
  const LarsSeg last = t.segs[seg_hi - 1];
  c1 = min(last.chunk0 + last.nchunks, t.nchunks);
}

// a chunk entry that would read or write outside the flat buffers is skipped, not trusted
__device__ __forceinline__ bool chunk_ok(const Table& t, const LarsChunk& ck) {
  const int seg = (int)((uint32_t)ck.seg & ~kExcludedBit);
  return ck.n > 0 && ck.n <= kLambChunk && ck.start >= 0 && ck.start + ck.n <= t.numel && seg < t.nseg;
}

// bias corrections of update number t: (1 - beta1^t, sqrt(1 - beta2^t)), float64 rounded to fp32
__device__ __forceinline__ void bias_corrections(int64_t t, double beta1, double beta2, float& bc1, float& sbc2) {
  bc1 = (float)(1.0 - pow(beta1, (double)t));
  sbc2 = (float)sqrt(1.0 - pow(beta2, (double)t));
}

__device__ __forceinline__ void moments(float g, float& m, float& v, const Coef& c) {
  m = fmaf(c.b1, m, c.omb1 * g);
  v = fmaf(c.b2, v, (c.omb2 * g) * g);
}

__device__ __forceinline__ float direction(float p, float m, float v, float wde, float bc1, float sbc2, float eps) {
  return fmaf(wde, p, (m / bc1) / (sqrtf(v) / sbc2 + eps));
}

// SINGLE: trust is off, every chunk is finished here and nothing is summed
// CLIP: the gradient is clip[kClipCoef] * g, rounded to fp32, before the moments
template <bool SINGLE, bool MIRROR, bool CLIP>
__global__ void __launch_bounds__(256) lamb_moments_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                           float* __restrict__ m, float* __restrict__ v, Table tb,
                                                           const LambRecord* __restrict__ rec,
                                                           double* __restrict__ partials, int seg_lo, int seg_hi,
                                                           Coef cf, double beta1, double beta2,
                                                           uint16_t* __restrict__ pb,
                                                           const float* __restrict__ clip) {
  __shared__ double red[8];
  __shared__ float bcs[2];
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  if (t == 0) bias_corrections(rec->done + 1, beta1, beta2, bcs[0], bcs[1]);
  __syncthreads();
  const float bc1 = bcs[0], sbc2 = bcs[1];
  const float coef = CLIP ? clip[kClipCoef] : 1.f;
  int c0, c1;
  chunk_range(tb, seg_lo, seg_hi, c0, c1);
  for (int c = c0 + (int)blockIdx.x; c < c1; c += (int)gridDim.x) {
    const LarsChunk ck = tb.chunks[c];
    if (!chunk_ok(tb, ck)) continue;
    const bool excl = ((uint32_t)ck.seg & kExcludedBit) != 0;
    const bool fin = SINGLE || excl;  // p is final after this pass
    const float wde = excl ? 0.f : cf.wd;
    const int64_t s = ck.start;
    const int n = ck.n;
    // `lead` elements before the first 16-B-aligned one, then float4, then the tail (as lars.hip)
    const int lead = min(n, (int)((4 - (s & 3)) & 3));
    double sp = 0.0, su = 0.0;
    auto step = [&](float& pp, float gg, float& mm, float& vv) {
      if (CLIP) gg = coef * gg;
      moments(gg, mm, vv, cf);
      const float u = direction(pp, mm, vv, wde, bc1, sbc2, cf.eps);
      if (!fin) {
        const double pd = (double)pp, ud = (double)u;
        sp = fma(pd, pd, sp);
        su = fma(ud, ud, su);
      }
      if (fin) pp = fmaf(cf.nlr, u, pp);
    };
    auto one = [&](int64_t i) {
      float pv = p[i], mv = m[i], vv = v[i];
      step(pv, g[i], mv, vv);
      m[i] = mv;
      v[i] = vv;
      if (fin) {
        p[i] = pv;
        if (MIRROR) pb[i] = f2bf(pv);
      }
    };
    if (t < lead) one(s + t);
    const int n4 = (n - lead) >> 2;
    float4* p4 = reinterpret_cast<float4*>(p + s + lead);
    const float4* g4 = reinterpret_cast<const float4*>(g + s + lead);
    float4* m4 = reinterpret_cast<float4*>(m + s + lead);
    float4* v4 = reinterpret_cast<float4*>(v + s + lead);
    uint2* pb4 = reinterpret_cast<uint2*>(pb + s + lead);
    for (int i = t; i < n4; i += 256) {
      float4 pv = p4[i], mv = m4[i], vv = v4[i];
      const float4 gv = g4[i];
      step(pv.x, gv.x, mv.x, vv.x); step(pv.y, gv.y, mv.y, vv.y);
      step(pv.z, gv.z, mv.z, vv.z); step(pv.w, gv.w, mv.w, vv.w);
      m4[i] = mv;
      v4[i] = vv;
      if (fin) {
        p4[i] = pv;
        if (MIRROR) pb4[i] = make_uint2(pack2bf(pv.x, pv.y), pack2bf(pv.z, pv.w));
      }
    }
    for (int i = lead + n4 * 4 + t; i < n; i += 256) one(s + i);
    if (!fin) {  // uniform over the block
      sp = wave_sum_f64(sp);
      su = wave_sum_f64(su);
      if (lane == 0) { red[wid] = sp; red[4 + wid] = su; }
      __syncthreads();
      if (t == 0) {
        partials[2 * (int64_t)c] = (red[0] + red[1]) + (red[2] + red[3]);
        partials[2 * (int64_t)c + 1] = (red[4] + red[5]) + (red[6] + red[7]);
      }
      __syncthreads();
    }
  }
}

// one wave per segment; lane 0 of block 0 alone touches the record
__global__ void __launch_bounds__(64) lamb_trust_kernel(Table tb, const double* __restrict__ partials,
                                                        float* __restrict__ trust, LambRecord* __restrict__ rec,
                                                        int seg_lo, double beta1, double beta2, bool advance,
                                                        bool trust_clip) {
  const int seg = seg_lo + (int)blockIdx.x;
  const int lane = threadIdx.x;
  if (blockIdx.x == 0 && lane == 0) {
    const int64_t t = rec->done + 1;
    float bc1, sbc2;
    bias_corrections(t, beta1, beta2, bc1, sbc2);
    rec->bc1 = bc1;
    rec->sbc2 = sbc2;
    if (advance) rec->done = t;
  }
  const LarsSeg e = tb.segs[seg];
  float tr = 1.f;
  if (!(e.flags & 1)) {
    double sp = 0.0, su = 0.0;
    for (int k = lane; k < e.nchunks; k += 64) {
      const int c = e.chunk0 + k;
      if (c < 0 || c >= tb.nchunks) continue;
      sp += partials[2 * (int64_t)c];
      su += partials[2 * (int64_t)c + 1];
    }
    sp = wave_sum_f64(sp);
    su = wave_sum_f64(su);
    if (!(sp == 0.0 || su == 0.0)) {
#pragma clang fp contract(off)  // round every operation, as the float64 reference does
      tr = (float)(sqrt(sp) / sqrt(su));
    }
    if (trust_clip && tr > 1.f) tr = 1.f;
  }
  if (lane == 0) trust[seg] = tr;
}

// AdamW: the counter advances in a launch of its own, behind the single pass that read it
__global__ void lamb_advance_kernel(LambRecord* __restrict__ rec) {
  if (blockIdx.x == 0 && threadIdx.x == 0) rec->done = rec->done + 1;
}

template <bool MIRROR>
__global__ void __launch_bounds__(256) lamb_update_kernel(float* __restrict__ p, const float* __restrict__ m,
                                                          const float* __restrict__ v, Table tb,
                                                          const float* __restrict__ trust,
                                                          const LambRecord* __restrict__ rec, int seg_lo, int seg_hi,
                                                          Coef cf, double lr, uint16_t* __restrict__ pb) {
  const int t = threadIdx.x;
  const float bc1 = rec->bc1, sbc2 = rec->sbc2;
  int c0, c1;
  chunk_range(tb, seg_lo, seg_hi, c0, c1);
  for (int c = c0 + (int)blockIdx.x; c < c1; c += (int)gridDim.x) {
    const LarsChunk ck = tb.chunks[c];
    if (!chunk_ok(tb, ck) || ((uint32_t)ck.seg & kExcludedBit)) continue;  // excluded: done in pass 1
    const float nstep = -(float)(lr * (double)trust[ck.seg]);
    const int64_t s = ck.start;
    const int n = ck.n;
    const int lead = min(n, (int)((4 - (s & 3)) & 3));
    auto step = [&](float& pp, float mm, float vv) {
      pp = fmaf(nstep, direction(pp, mm, vv, cf.wd, bc1, sbc2, cf.eps), pp);
    };
    auto one = [&](int64_t i) {
      float pv = p[i];
      step(pv, m[i], v[i]);
      p[i] = pv;
      if (MIRROR) pb[i] = f2bf(pv);
    };
    if (t < lead) one(s + t);
    const int n4 = (n - lead) >> 2;
    float4* p4 = reinterpret_cast<float4*>(p + s + lead);
    const float4* m4 = reinterpret_cast<const float4*>(m + s + lead);
    const float4* v4 = reinterpret_cast<const float4*>(v + s + lead);
    uint2* pb4 = reinterpret_cast<uint2*>(pb + s + lead);
    for (int i = t; i < n4; i += 256) {
      float4 pv = p4[i];
      const float4 mv = m4[i], vv = v4[i];
      step(pv.x, mv.x, vv.x); step(pv.y, mv.y, vv.y); step(pv.z, mv.z, vv.z); step(pv.w, mv.w, vv.w);
      p4[i] = pv;
      if (MIRROR) pb4[i] = make_uint2(pack2bf(pv.x, pv.y), pack2bf(pv.z, pv.w));
    }
    for (int i = lead + n4 * 4 + t; i < n; i += 256) one(s + i);
  }
}

static Table table_of(const LambSpace& sp, int seg_lo, int seg_hi) {
  if (!sp.table || !sp.rec || sp.nseg <= 0 || sp.nchunks < 0 || seg_lo < 0 || seg_hi > sp.nseg)
    throw std::runtime_error("lamb: segment range outside the table");
  Table t;
  t.segs = static_cast<const LarsSeg*>(sp.table);
  t.chunks = reinterpret_cast<const LarsChunk*>(t.segs + sp.nseg);
  t.nseg = sp.nseg;
  t.nchunks = sp.nchunks;
  t.numel = sp.numel;
  return t;
}

static unsigned chunk_grid(const LambSpace& sp, int max_chunks) {
  // memory-bound: at most 8 blocks per CU resident, the rest of the chunks by grid stride
  return (unsigned)std::max(1, std::min(std::min(max_chunks, sp.nchunks), 2048));
}

static bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

static void check_bufs(const LambBufs& b, bool need_g) {
  if (!b.p || !b.m || !b.v || (need_g && !b.g)) throw std::runtime_error("lamb: missing flat buffer");
  if (!aligned16(b.p) || !aligned16(b.g) || !aligned16(b.m) || !aligned16(b.v) || !aligned16(b.mirror))
    throw std::runtime_error("lamb: flat buffers must be 16-byte aligned");
}

static Coef coef_of(const LambHyper& h) {
  Coef c;
  c.b1 = (float)h.beta1;
  c.omb1 = (float)(1.0 - h.beta1);
  c.b2 = (float)h.beta2;
  c.omb2 = (float)(1.0 - h.beta2);
  c.eps = (float)h.eps;
  c.wd = (float)h.wd;
  c.nlr = -(float)h.lr;
  return c;
}

template <bool SINGLE, bool CLIP>
static void launch_moments_c(const LambBufs& b, const LambSpace& sp, int seg_lo, int seg_hi, int max_chunks,
                             const LambHyper& h, hipStream_t st) {
  Table tb = table_of(sp, seg_lo, seg_hi);
  check_bufs(b, true);
  if (!SINGLE && !sp.partials) throw std::runtime_error("lamb: missing partials");
  dim3 gr(chunk_grid(sp, max_chunks)), bl(256);
  const Coef cf = coef_of(h);
  if (b.mirror)
    hipLaunchKernelGGL((lamb_moments_kernel<SINGLE, true, CLIP>), gr, bl, 0, st, b.p, b.g, b.m, b.v, tb, sp.rec,
                       sp.partials, seg_lo, seg_hi, cf, h.beta1, h.beta2, b.mirror, b.clip);
  else
    hipLaunchKernelGGL((lamb_moments_kernel<SINGLE, false, CLIP>), gr, bl, 0, st, b.p, b.g, b.m, b.v, tb, sp.rec,
                       sp.partials, seg_lo, seg_hi, cf, h.beta1, h.beta2, (uint16_t*)nullptr, b.clip);
}

template <bool SINGLE>
static void launch_moments_t(const LambBufs& b, const LambSpace& sp, int seg_lo, int seg_hi, int max_chunks,
                             const LambHyper& h, hipStream_t st) {
  if (b.clip)
    launch_moments_c<SINGLE, true>(b, sp, seg_lo, seg_hi, max_chunks, h, st);
  else
    launch_moments_c<SINGLE, false>(b, sp, seg_lo, seg_hi, max_chunks, h, st);
}

void launch_lamb_moments(const LambBufs& b, const LambSpace& sp, int seg_lo, int seg_hi, int max_chunks,
                         const LambHyper& h, hipStream_t st) {
  if (seg_hi <= seg_lo) return;
  launch_moments_t<false>(b, sp, seg_lo, seg_hi, max_chunks, h, st);
}

void launch_lamb_trust(const LambSpace& sp, int seg_lo, int seg_hi, const LambHyper& h, bool advance,
                       hipStream_t st) {
  if (seg_hi <= seg_lo) return;
  Table tb = table_of(sp, seg_lo, seg_hi);
  if (!sp.partials || !sp.trust) throw std::runtime_error("lamb: missing partials / trust");
  hipLaunchKernelGGL(lamb_trust_kernel, dim3((unsigned)(seg_hi - seg_lo)), dim3(64), 0, st, tb, sp.partials,
                     sp.trust, sp.rec, seg_lo, h.beta1, h.beta2, advance, h.trust_clip);
}

void launch_lamb_update(const LambBufs& b, const LambSpace& sp, int seg_lo, int seg_hi, int max_chunks,
                        const LambHyper& h, hipStream_t st) {
  if (seg_hi <= seg_lo) return;
  Table tb = table_of(sp, seg_lo, seg_hi);
  check_bufs(b, false);
  if (!sp.trust) throw std::runtime_error("lamb: missing trust");
  dim3 gr(chunk_grid(sp, max_chunks)), bl(256);
  const Coef cf = coef_of(h);
  if (b.mirror)
    hipLaunchKernelGGL((lamb_update_kernel<true>), gr, bl, 0, st, b.p, b.m, b.v, tb, sp.trust, sp.rec, seg_lo,
                       seg_hi, cf, h.lr, b.mirror);
  else
    hipLaunchKernelGGL((lamb_update_kernel<false>), gr, bl, 0, st, b.p, b.m, b.v, tb, sp.trust, sp.rec, seg_lo,
                       seg_hi, cf, h.lr, (uint16_t*)nullptr);
}

void launch_lamb(const LambBufs& b, const LambSpace& sp, int seg_lo, int seg_hi, int max_chunks,
                 const LambHyper& h, bool advance, hipStream_t st) {
  launch_lamb_moments(b, sp, seg_lo, seg_hi, max_chunks, h, st);
  launch_lamb_trust(sp, seg_lo, seg_hi, h, advance, st);
  launch_lamb_update(b, sp, seg_lo, seg_hi, max_chunks, h, st);
}

void launch_adamw(const LambBufs& b, const LambSpace& sp, int seg_lo, int seg_hi, int max_chunks,
                  const LambHyper& h, bool advance, hipStream_t st) {
  if (seg_hi <= seg_lo) return;
  launch_moments_t<true>(b, sp, seg_lo, seg_hi, max_chunks, h, st);
  if (advance) hipLaunchKernelGGL(lamb_advance_kernel, dim3(1), dim3(1), 0, st, sp.rec);
}

}  // namespace pdt::opt
