// Exponential moving average of the weights over the flat storage: e <- e + w * (p - e), w = 1 - decay.
//
// torch.optim.swa_utils.AveragedModel issues a _foreach_lerp_ over 161 (ResNet-50) parameter tensors
// and ~106 float buffers plus a copy per integer buffer; here the model's parameters are one flat
// fp32 buffer, its float buffers one flat tensor and its counters one flat int64 tensor, and the
// averaged twin keeps the same three layouts, so the whole update is ONE streaming launch: per
// parameter 2 reads + 1 write of fp32 and, like the fused SGD step (csrc/kernels/sgd.hip), a bf16
// side output -- conv weights in flat order already are KRSC, so bf16(e') at the same offset is the
// twin's forward weight mirror.  14 B per parameter.
//
// Same shape as sgd_kernel: 16-byte accesses in the body, a scalar lead up to the first
// 16-byte-aligned element and a scalar tail, 64-bit indices, a capped grid with a grid-stride loop.
// The three segments run one after the other in the same launch (the float buffers are ~0.2 % of
// the parameters, the counters a few dozen elements).
//
// Plain loads and stores: the three streams are touched once per update, so non-temporal accesses
// (__builtin_nontemporal_load/store on all of them) were tried to keep the next forward's weights in
// L2 / Infinity Cache; they were 15 % slower alone and no faster in the step (README "Weight EMA",
// profiles/ema_nt_ab.json), and were dropped.
#include "ema.h"

#include <algorithm>
#include <stdexcept>
#include <string>

#include "kernels/common.h"

namespace pdt::ema {

typedef float ema_f4 __attribute__((ext_vector_type(4)));
typedef uint32_t ema_u2 __attribute__((ext_vector_type(2)));

// w == 1 and w == 0 are exact by selection (e + 1 * (p - e) rounds twice): the first update of a
// ModelEma is a copy, and a frozen EMA must not drift
__device__ __forceinline__ float blend(float e, float p, float w) {
  float r = fmaf(w, p - e, e);
  r = w == 1.f ? p : r;
  return w == 0.f ? e : r;
}

// `lead` elements before the first 16-byte-aligned one of e (p shares the phase, bf + lead is
// 8-byte aligned: lerp_seg_error) and the tail go one at a time; the body in 4-element vectors
template <bool BF>
__device__ __forceinline__ void lerp_range(float* e, const float* p, uint16_t* bf, int64_t n, int lead, float w,
                                           int64_t tid, int64_t stride) {
  auto one = [&](int64_t i) {
    float r = blend(e[i], p[i], w);
    e[i] = r;
    if (BF) bf[i] = f2bf(r);
  };
  if (tid < lead) one(tid);  // lead <= n
  const int64_t n4 = (n - lead) / 4;
  ema_f4* e4 = reinterpret_cast<ema_f4*>(e + lead);
  const ema_f4* p4 = reinterpret_cast<const ema_f4*>(p + lead);
  ema_u2* b2 = BF ? reinterpret_cast<ema_u2*>(bf + lead) : nullptr;
  for (int64_t i = tid; i < n4; i += stride) {
    ema_f4 ev = e4[i];
    ema_f4 pv = p4[i];
    ema_f4 r;
    r.x = blend(ev.x, pv.x, w); r.y = blend(ev.y, pv.y, w);
    r.z = blend(ev.z, pv.z, w); r.w = blend(ev.w, pv.w, w);
    e4[i] = r;
    if (BF) {
      ema_u2 b;
      b.x = pack2bf(r.x, r.y); b.y = pack2bf(r.z, r.w);
      b2[i] = b;
    }
  }
  for (int64_t i = lead + n4 * 4 + tid; i < n; i += stride) one(i);
}

template <bool BF>
__global__ void __launch_bounds__(256) ema_kernel(LerpSeg a, int lead_a, LerpSeg b, int lead_b, CopySeg c,
                                                  float w) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (a.n > 0) lerp_range<BF>(a.e, a.p, a.bf, a.n, lead_a, w, tid, stride);
  if (b.n > 0) lerp_range<false>(b.e, b.p, nullptr, b.n, lead_b, w, tid, stride);
  for (int64_t i = tid; i < c.n; i += stride) c.dst[i] = c.src[i];
}

static int lead_of(const void* q) { return (int)(((16 - ((uintptr_t)q & 15)) & 15) >> 2); }

const char* lerp_seg_error(const LerpSeg& s) {
  if (!s.e && !s.p) return nullptr;
  if (((uintptr_t)s.e & 3) || ((uintptr_t)s.p & 3)) return "fp32 buffers must be 4-byte aligned";
  if (((uintptr_t)s.e & 15) != ((uintptr_t)s.p & 15))
    return "the EMA and the model buffer must share their 16-byte phase (the kernel moves 16-byte vectors of both)";
  if (s.bf && ((uintptr_t)(s.bf + lead_of(s.e)) & 7))
    return "the bf16 output must be 8-byte aligned where the EMA buffer is 16-byte aligned";
  return nullptr;
}

void launch_ema_update(const LerpSeg& params, const LerpSeg& buffers, const CopySeg& counters, float w,
                       hipStream_t st) {
  if (buffers.bf) throw std::runtime_error("ema_update: the buffer segment has no bf16 output");
  for (const LerpSeg* s : {&params, &buffers})
    if (const char* err = lerp_seg_error(*s)) throw std::runtime_error(std::string("ema_update: ") + err);
  if (params.n <= 0 && buffers.n <= 0 && counters.n <= 0) return;
  const int lead_a = (int)std::min<int64_t>(std::max<int64_t>(params.n, 0), lead_of(params.e));
  const int lead_b = (int)std::min<int64_t>(std::max<int64_t>(buffers.n, 0), lead_of(buffers.e));
  int64_t blocks = (std::max(params.n, buffers.n) / 4 + 255) / 256;
  blocks = std::min<int64_t>(std::max<int64_t>(blocks, 1), 4096);
  dim3 gr((unsigned)blocks), bl(256);
  const bool bf = params.bf != nullptr && params.n > 0;
  if (bf) hipLaunchKernelGGL((ema_kernel<true>), gr, bl, 0, st, params, lead_a, buffers, lead_b, counters, w);
  else hipLaunchKernelGGL((ema_kernel<false>), gr, bl, 0, st, params, lead_a, buffers, lead_b, counters, w);
}

}  // namespace pdt::ema
