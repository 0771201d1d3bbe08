// LARS (layer-wise adaptive rate scaling) over ONE flat fp32 parameter buffer, in the "rescale the
// gradient, then SGD" form, so the momentum buffer keeps torch.optim.SGD's meaning:
//   trust = excluded or |p| == 0 or |g| == 0 ? 1 : float(eta |p| / (|g| + wd |p| + eps))   (float64)
//   d = trust * (g + wd_eff p) ; buf = first ? d : m*buf + (1-damp)*d ;
//   d = nesterov ? d + m*buf : buf ; p -= lr*d                        (wd_eff = excluded ? 0 : wd)
// Three streaming-friendly passes over a table of segments (one per parameter tensor) cut into
// chunks of at most kChunk elements:
//   norms  : one block per chunk writes (sum p^2, sum g^2) in float64 to partials[chunk];
//   trust  : one wave per segment sums its chunks' partials and writes trust[seg];
//   update : one block per chunk, the element math of sgd_kernel with trust[seg] and wd_eff.
// No floating-point atomics: the tree inside a chunk (per-thread order, wave butterfly, 4 waves) and
// the order over a segment's chunks (lane k sums chunks k, k+64, ..., then the butterfly) are fixed by
// the table alone.  The grid size, the stream and the segment range [seg_lo, seg_hi) a launch covers
// only decide WHICH block handles a chunk, never how it is summed -- every rank of a data-parallel
// job gets bitwise-identical trust ratios from its copy of an all-reduced bucket, and a space
// processed per bucket equals the space processed in one go.
#include "common.h"
#include "kernels.h"

#include <algorithm>
#include <stdexcept>

namespace pdt {

constexpr int kChunk = 4096;  // elements: 4 float4 per lane of a 256-thread block
constexpr uint32_t kExcludedBit = 0x80000000u;  // LarsChunk::seg bit 31 = the segment's flag bit 0

size_t lars_entry_bytes() { return sizeof(LarsSeg); }
size_t lars_chunk_entry_bytes() { return sizeof(LarsChunk); }
int lars_chunk_elems() { return kChunk; }

struct LarsTable {
  const LarsSeg* segs;
  const LarsChunk* chunks;
  int nseg, nchunks;
  int64_t numel;
};

// chunk range of the segments [seg_lo, seg_hi) (the launchers checked 0 <= seg_lo < seg_hi <= nseg)
__device__ __forceinline__ void chunk_range(const LarsTable& t, int seg_lo, int seg_hi, int& c0, int& c1) {
  c0 = max(t.segs[seg_lo].chunk0, 0);
  const LarsSeg last = t.segs[seg_hi - 1];
  c1 = min(last.chunk0 + last.nchunks, t.nchunks);
}

// a chunk entry that would read or write outside the flat buffers is skipped, not trusted
__device__ __forceinline__ bool chunk_ok(const LarsTable& t, const LarsChunk& ck) {
  const int seg = (int)((uint32_t)ck.seg & ~kExcludedBit);
  return ck.n > 0 && ck.n <= kChunk && ck.start >= 0 && ck.start + ck.n <= t.numel && seg < t.nseg;
}

__global__ void __launch_bounds__(256) lars_norms_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                         LarsTable tb, double* __restrict__ partials,
                                                         int seg_lo, int seg_hi) {
  __shared__ double red[8];
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  int c0, c1;
  chunk_range(tb, seg_lo, seg_hi, c0, c1);
  for (int c = c0 + (int)blockIdx.x; c < c1; c += (int)gridDim.x) {
    const LarsChunk ck = tb.chunks[c];
    if (!chunk_ok(tb, ck) || ((uint32_t)ck.seg & kExcludedBit)) continue;  // excluded: trust is 1
    const int64_t s = ck.start;
    const int n = ck.n;
    // `lead` elements before the first 16-B-aligned one, then float4, then the tail (as sgd_kernel)
    const int lead = min(n, (int)((4 - (s & 3)) & 3));
    double sp = 0.0, sg = 0.0;
    auto acc = [&](float pv, float gv) {
      const double pd = (double)pv, gd = (double)gv;
      sp = fma(pd, pd, sp);
      sg = fma(gd, gd, sg);
    };
    if (t < lead) acc(p[s + t], g[s + t]);
    const int n4 = (n - lead) >> 2;
    const float4* p4 = reinterpret_cast<const float4*>(p + s + lead);
    const float4* g4 = reinterpret_cast<const float4*>(g + s + lead);
    for (int i = t; i < n4; i += 256) {
      const float4 pv = p4[i], gv = g4[i];
      acc(pv.x, gv.x); acc(pv.y, gv.y); acc(pv.z, gv.z); acc(pv.w, gv.w);
    }
    for (int i = lead + n4 * 4 + t; i < n; i += 256) acc(p[s + i], g[s + i]);
    sp = wave_sum_f64(sp);
    sg = wave_sum_f64(sg);
    if (lane == 0) { red[wid] = sp; red[4 + wid] = sg; }
    __syncthreads();
    if (t == 0) {
      partials[2 * (int64_t)c] = (red[0] + red[1]) + (red[2] + red[3]);
      partials[2 * (int64_t)c + 1] = (red[4] + red[5]) + (red[6] + red[7]);
    }
    __syncthreads();
  }
}

// one wave per segment
__global__ void __launch_bounds__(64) lars_trust_kernel(LarsTable tb, const double* __restrict__ partials,
                                                        float* __restrict__ trust, int seg_lo, double wd,
                                                        double eta, double eps) {
  const int seg = seg_lo + (int)blockIdx.x;
  const int lane = threadIdx.x;
  const LarsSeg e = tb.segs[seg];
  float tr = 1.f;
  if (!(e.flags & 1)) {
    double sp = 0.0, sg = 0.0;
    for (int k = lane; k < e.nchunks; k += 64) {
      const int c = e.chunk0 + k;
      if (c < 0 || c >= tb.nchunks) continue;
      sp += partials[2 * (int64_t)c];
      sg += partials[2 * (int64_t)c + 1];
    }
    sp = wave_sum_f64(sp);
    sg = wave_sum_f64(sg);
    if (!(sp == 0.0 || sg == 0.0)) {
#pragma clang fp contract(off)  // round every operation, as the float64 reference does
      const double pn = sqrt(sp), gn = sqrt(sg);
      tr = (float)((eta * pn) / ((gn + wd * pn) + eps));
    }
  }
  if (lane == 0) trust[seg] = tr;
}

template <bool MOM, bool NEST, bool MIRROR>
__global__ void __launch_bounds__(256) lars_update_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                          float* __restrict__ buf, LarsTable tb,
                                                          const float* __restrict__ trust, int seg_lo,
                                                          int seg_hi, float lr, float mom, float damp1,
                                                          float wd, bool first, uint16_t* __restrict__ pb) {
  const int t = threadIdx.x;
  int c0, c1;
  chunk_range(tb, seg_lo, seg_hi, c0, c1);
  for (int c = c0 + (int)blockIdx.x; c < c1; c += (int)gridDim.x) {
    const LarsChunk ck = tb.chunks[c];
    if (!chunk_ok(tb, ck)) continue;
    const uint32_t sx = (uint32_t)ck.seg;
    const float tr = trust[sx & ~kExcludedBit];
    const float wde = (sx & kExcludedBit) ? 0.f : wd;
    const int64_t s = ck.start;
    const int n = ck.n;
    const int lead = min(n, (int)((4 - (s & 3)) & 3));
    auto step = [&](float& pp, float gg, float& bb) {
      float d = tr * fmaf(wde, pp, gg);
      if (MOM) {
        bb = first ? d : fmaf(mom, bb, damp1 * d);
        d = NEST ? fmaf(mom, bb, d) : bb;
      }
      pp = fmaf(-lr, d, pp);
    };
    auto one = [&](int64_t i) {
      float pv = p[i], bv = MOM ? buf[i] : 0.f;
      step(pv, g[i], bv);
      p[i] = pv;
      if (MOM) buf[i] = bv;
      if (MIRROR) pb[i] = f2bf(pv);
    };
    if (t < lead) one(s + t);
    const int n4 = (n - lead) >> 2;
    float4* p4 = reinterpret_cast<float4*>(p + s + lead);
    const float4* g4 = reinterpret_cast<const float4*>(g + s + lead);
    float4* b4 = reinterpret_cast<float4*>(buf + s + lead);
    uint2* pb4 = reinterpret_cast<uint2*>(pb + s + lead);
    for (int i = t; i < n4; i += 256) {
      float4 pv = p4[i];
      float4 gv = g4[i];
      float4 bv = MOM ? b4[i] : make_float4(0, 0, 0, 0);
      step(pv.x, gv.x, bv.x); step(pv.y, gv.y, bv.y); step(pv.z, gv.z, bv.z); step(pv.w, gv.w, bv.w);
      p4[i] = pv;
      if (MOM) b4[i] = bv;
      if (MIRROR) pb4[i] = make_uint2(pack2bf(pv.x, pv.y), pack2bf(pv.z, pv.w));
    }
    for (int i = lead + n4 * 4 + t; i < n; i += 256) one(s + i);
  }
}

static LarsTable table_of(const LarsSpace& sp, int seg_lo, int seg_hi) {
  if (!sp.table || sp.nseg <= 0 || sp.nchunks < 0 || seg_lo < 0 || seg_hi > sp.nseg)
    throw std::runtime_error("lars: segment range outside the table");
  LarsTable t;
  t.segs = static_cast<const LarsSeg*>(sp.table);
  t.chunks = reinterpret_cast<const LarsChunk*>(t.segs + sp.nseg);
  t.nseg = sp.nseg;
  t.nchunks = sp.nchunks;
  t.numel = sp.numel;
  return t;
}

static unsigned chunk_grid(const LarsSpace& sp, int max_chunks) {
  // memory-bound: at most 8 blocks per CU resident, the rest of the chunks by grid stride
  return (unsigned)std::max(1, std::min(std::min(max_chunks, sp.nchunks), 2048));
}

static bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

void launch_lars_norms(const float* p, const float* g, const LarsSpace& sp, int seg_lo, int seg_hi,
                       int max_chunks, hipStream_t st) {
  if (seg_hi <= seg_lo) return;
  LarsTable tb = table_of(sp, seg_lo, seg_hi);
  if (!aligned16(p) || !aligned16(g)) throw std::runtime_error("lars: flat buffers must be 16-byte aligned");
  hipLaunchKernelGGL(lars_norms_kernel, dim3(chunk_grid(sp, max_chunks)), dim3(256), 0, st, p, g, tb,
                     sp.partials, seg_lo, seg_hi);
}

void launch_lars_trust(const LarsSpace& sp, int seg_lo, int seg_hi, double wd, double eta, double eps,
                       hipStream_t st) {
  if (seg_hi <= seg_lo) return;
  LarsTable tb = table_of(sp, seg_lo, seg_hi);
  hipLaunchKernelGGL(lars_trust_kernel, dim3((unsigned)(seg_hi - seg_lo)), dim3(64), 0, st, tb, sp.partials,
                     sp.trust, seg_lo, wd, eta, eps);
}

template <bool MIRROR>
static void launch_lars_update_t(float* p, const float* g, float* buf, const LarsTable& tb, const float* trust,
                                 unsigned grid, int seg_lo, int seg_hi, float lr, float momentum,
                                 float dampening, float wd, bool nesterov, bool first, hipStream_t st,
                                 uint16_t* pb) {
  dim3 gr(grid), bl(256);
  const float damp1 = 1.f - dampening;
  if (momentum == 0.f)
    hipLaunchKernelGGL((lars_update_kernel<false, false, MIRROR>), gr, bl, 0, st, p, g, buf, tb, trust, seg_lo, seg_hi, lr, momentum, damp1, wd, first, pb);
  else if (nesterov)
    hipLaunchKernelGGL((lars_update_kernel<true, true, MIRROR>), gr, bl, 0, st, p, g, buf, tb, trust, seg_lo, seg_hi, lr, momentum, damp1, wd, first, pb);
  else
    hipLaunchKernelGGL((lars_update_kernel<true, false, MIRROR>), gr, bl, 0, st, p, g, buf, tb, trust, seg_lo, seg_hi, lr, momentum, damp1, wd, first, pb);
}

void launch_lars_update(float* p, const float* g, float* buf, const LarsSpace& sp, int seg_lo, int seg_hi,
                        int max_chunks, float lr, float momentum, float dampening, float wd, bool nesterov,
                        bool first, hipStream_t st, uint16_t* p_bf16) {
  if (seg_hi <= seg_lo) return;
  LarsTable tb = table_of(sp, seg_lo, seg_hi);
  if (!aligned16(p) || !aligned16(g) || (momentum != 0.f && (!buf || !aligned16(buf))) ||
      (p_bf16 && !aligned16(p_bf16)))
    throw std::runtime_error("lars: flat buffers must be 16-byte aligned");
  const unsigned grid = chunk_grid(sp, max_chunks);
  if (p_bf16)
    launch_lars_update_t<true>(p, g, buf, tb, sp.trust, grid, seg_lo, seg_hi, lr, momentum, dampening, wd, nesterov, first, st, p_bf16);
  else
    launch_lars_update_t<false>(p, g, buf, tb, sp.trust, grid, seg_lo, seg_hi, lr, momentum, dampening, wd, nesterov, first, st, nullptr);
}

void launch_lars(float* p, const float* g, float* buf, const LarsSpace& sp, int seg_lo, int seg_hi,
                 int max_chunks, float lr, float momentum, float dampening, double wd, bool nesterov,
                 bool first, double eta, double eps, hipStream_t st, uint16_t* p_bf16) {
  launch_lars_norms(p, g, sp, seg_lo, seg_hi, max_chunks, st);
  launch_lars_trust(sp, seg_lo, seg_hi, wd, eta, eps, st);
  launch_lars_update(p, g, buf, sp, seg_lo, seg_hi, max_chunks, lr, momentum, dampening, (float)wd, nesterov,
                     first, st, p_bf16);
}

}  // namespace pdt
