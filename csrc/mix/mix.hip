// MixUp / CutMix on the device, folded into the two passes the training step already makes over
// the batch and over the logits (semantics: data/mix.py and ops/reference.py::softmax_xent_mix).
//
// augment_mix_kernel is augment_kernel (csrc/kernels/augment.hip) with a second source: a pixel in
// the sample's CutMix box is gathered through the PARTNER's own index, crop offsets and flip, and
// a blended sample (w != 1) gathers both pixels.  One pass, one 16-byte store per lane.  Without
// a blend every pixel has exactly one source, chosen BEFORE the load, so a wave that straddles a
// box edge still issues one gather per pixel (no divergent second gather); a wave none of whose
// lanes touches a box runs augment_kernel's own loop, and an unmixed sample never touches its
// partner.
//
// softmax_xent_mix_kernel is softmax_xent_kernel (csrc/kernels/head.hip) with the target
// lam * onehot(a) + (1 - lam) * onehot(b).  With lam == 1 it reproduces that kernel bit for bit.
//
// Floating-point contraction is OFF for this file.  The blend a*w + p*(1-w) rounds both products
// on their own (as the ATen chain of data/mix.py does), and the one fused multiply-add the loss
// head needs to match softmax_xent_kernel (whose `e * inv_s - target` the compiler contracts) is
// written out as fmaf.
#include "mix.h"

#include <stdexcept>

#include "kernels/common.h"

#pragma clang fp contract(off)

namespace pdt::mix {

template <bool U8, bool NORM>
__device__ __forceinline__ float gather_px(const void* __restrict__ src_, int64_t n, int c, int sy, int sx, int C,
                                           int H, int W, float mean, float stdv) {
  float p = 0.f;
  if ((unsigned)sy < (unsigned)H && (unsigned)sx < (unsigned)W) {
    const int64_t o = ((n * C + c) * H + sy) * W + sx;
    if constexpr (U8) p = (float)reinterpret_cast<const uint8_t*>(src_)[o] * (1.0f / 255.0f);
    else p = reinterpret_cast<const float*>(src_)[o];
  }
  if constexpr (NORM) p = (p - mean) / stdv;
  return p;
}

template <bool U8, bool NORM>
__global__ void __launch_bounds__(256) augment_mix_kernel(
    const void* __restrict__ src_, const int64_t* __restrict__ idx, const int64_t* __restrict__ oy,
    const int64_t* __restrict__ ox, const bool* __restrict__ flip, const int64_t* __restrict__ partner,
    const float* __restrict__ wgt, const int32_t* __restrict__ box, float* __restrict__ out, int B, int C, int H,
    int W, int pad, float m0, float m1, float m2, float s0, float s1, float s2) {
  const int W4 = W / 4;
  const int64_t total = (int64_t)B * C * H * W4;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int x4 = (int)(t % W4);
  int64_t r = t / W4;
  const int y = (int)(r % H);
  r /= H;
  const int c = (int)(r % C);
  const int b = (int)(r / C);
  const float mean = c == 0 ? m0 : (c == 1 ? m1 : m2);
  const float stdv = c == 0 ? s0 : (c == 1 ? s1 : s2);
  const float wb = wgt[b];
  const int4 bx = reinterpret_cast<const int4*>(box)[b];  // y1, y2, x1, x2
  const int xs = x4 * 4;
  const bool row_in = y >= bx.x && y < bx.y;
  const bool any_in = row_in && xs < bx.w && xs + 4 > bx.z;  // the store touches the box
  const bool blend = wb != 1.f;
  // gather parameters of the sample and, where the partner is needed at all, of the partner
  const int64_t n0 = idx[b];
  const int sy0 = y + (int)oy[b] - pad;
  const bool fl0 = flip != nullptr && flip[b];
  const int o0 = (int)ox[b] - pad;
  int64_t n1 = n0;
  int sy1 = sy0, o1 = o0;
  bool fl1 = fl0;
  if (any_in || blend) {
    int64_t pb = partner[b];
    if ((uint64_t)pb >= (uint64_t)B) pb = b;  // never index past the batch
    n1 = idx[pb];
    sy1 = y + (int)oy[pb] - pad;
    fl1 = flip != nullptr && flip[pb];
    o1 = (int)ox[pb] - pad;
  }
  float v[4];
  const bool wave_box = __any(any_in);  // wave-uniform, so the two unblended loops never both run
  if (!blend && !wave_box) {            // no lane of the wave touches a box: augment_kernel's loop
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int x = xs + q;
      v[q] = gather_px<U8, NORM>(src_, n0, c, sy0, (fl0 ? (W - 1 - x) : x) + o0, C, H, W, mean, stdv);
    }
  } else if (!blend) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int x = xs + q;
      const bool in = row_in && x >= bx.z && x < bx.w;
      v[q] = gather_px<U8, NORM>(src_, in ? n1 : n0, c, in ? sy1 : sy0,
                                 ((in ? fl1 : fl0) ? (W - 1 - x) : x) + (in ? o1 : o0), C, H, W, mean, stdv);
    }
  } else {
    const float wp = 1.f - wb;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int x = xs + q;
      const float a = gather_px<U8, NORM>(src_, n0, c, sy0, (fl0 ? (W - 1 - x) : x) + o0, C, H, W, mean, stdv);
      const float p = gather_px<U8, NORM>(src_, n1, c, sy1, (fl1 ? (W - 1 - x) : x) + o1, C, H, W, mean, stdv);
      v[q] = (row_in && x >= bx.z && x < bx.w) ? p : a * wb + p * wp;  // two roundings, then the add
    }
  }
  *reinterpret_cast<float4*>(out + t * 4) = make_float4(v[0], v[1], v[2], v[3]);
}

void launch_augment_mix(const void* src, bool src_u8, const int64_t* idx, const int64_t* oy, const int64_t* ox,
                        const bool* flip, const int64_t* partner, const float* w, const int32_t* box, float* out,
                        int B, int C, int H, int W, int pad, bool normalize, const float* mean, const float* stdv,
                        hipStream_t st) {
  if (W % 4 != 0) throw std::runtime_error("augment_mix: width must be a multiple of 4");
  if (C > 3) throw std::runtime_error("augment_mix: at most 3 channels");
  const int64_t total = (int64_t)B * C * H * (W / 4);
  if (total == 0) return;
  const unsigned blocks = (unsigned)((total + 255) / 256);
#define PDT_AUG_MIX(U8, NRM)                                                                             \
  hipLaunchKernelGGL((augment_mix_kernel<U8, NRM>), dim3(blocks), dim3(256), 0, st, src, idx, oy, ox, flip, \
                     partner, w, box, out, B, C, H, W, pad, mean[0], mean[1], mean[2], stdv[0], stdv[1], stdv[2])
  if (src_u8) { if (normalize) PDT_AUG_MIX(true, true); else PDT_AUG_MIX(true, false); }
  else { if (normalize) PDT_AUG_MIX(false, true); else PDT_AUG_MIX(false, false); }
#undef PDT_AUG_MIX
}

// One 256-thread block per row: max, sum of exponentials (and of the logits when SMOOTH), then
// the gradient -- the passes of softmax_xent_kernel in its order, so the sums are its sums.
// The target weights are ta = hit * lam on column a and tb = hit * (1 - lam) on column b, added
// where a == b.  lam == 1 gives ta = hit, tb = 0 exactly: every expression below then takes the
// value softmax_xent_kernel computes, whatever labels_b holds.
template <bool SMOOTH>
__global__ void __launch_bounds__(256) softmax_xent_mix_kernel(
    const float* __restrict__ logits, const int64_t* __restrict__ labels_a, const int64_t* __restrict__ labels_b,
    const float* __restrict__ lam, float* __restrict__ dlogits, float* __restrict__ row_loss, int V, float invN,
    float eps) {
  __shared__ float red[4];
  __shared__ float redx[4];
  const int row = blockIdx.x;
  const float* x = logits + (int64_t)row * V;
  float* g = dlogits + (int64_t)row * V;
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  float m = -INFINITY;
  for (int i = t; i < V; i += 256) m = fmaxf(m, x[i]);
  m = wave_max(m);
  if (lane == 0) red[wid] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  float s = 0.f, sx = 0.f;
  for (int i = t; i < V; i += 256) {
    const float xi = x[i];
    s += __expf(xi - m);
    if (SMOOTH) sx += xi;
  }
  s = wave_sum(s);
  if (SMOOTH) sx = wave_sum(sx);
  if (lane == 0) {
    red[wid] = s;
    if (SMOOTH) redx[wid] = sx;
  }
  __syncthreads();
  s = red[0] + red[1] + red[2] + red[3];
  const float inv_s = 1.f / s;
  const int64_t la = labels_a[row], lb = labels_b[row];
  const float l = lam[row];
  const float hit = SMOOTH ? 1.f - eps : 1.f;
  const float ta = hit * l, tb = hit * (1.f - l);
  const float miss = eps / (float)V;
  for (int i = t; i < V; i += 256) {
    const float tgt = (i == la ? ta : 0.f) + (i == lb ? tb : 0.f);
    float d = fmaf(__expf(x[i] - m), inv_s, -tgt);  // softmax_xent_kernel's contracted p - target
    if (SMOOTH) d -= miss;
    g[i] = d * invN;
  }
  if (t == 0) {
    const float lse = logf(s) + m;
    const float nll = l * (lse - x[la]) + (1.f - l) * (lse - x[lb]);
    if (SMOOTH) {
      sx = redx[0] + redx[1] + redx[2] + redx[3];
      row_loss[row] = hit * nll + eps * (lse - sx / (float)V);
    } else {
      row_loss[row] = nll;
    }
  }
}

// deterministic mean of the per-row losses (single block): the twin of head.hip's mean_kernel,
// whose launcher this module cannot reach
__global__ void __launch_bounds__(256) mix_mean_kernel(const float* __restrict__ v, int n, float* __restrict__ out) {
  __shared__ float red[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += v[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = (red[0] + red[1] + red[2] + red[3]) / (float)n;
}

void launch_softmax_xent_mix(const float* logits, const int64_t* labels_a, const int64_t* labels_b,
                             const float* lam, float* loss, float* dlogits, float* ws, int N, int V,
                             hipStream_t st, float label_smoothing) {
  if (N <= 0) throw std::runtime_error("softmax_xent_mix: empty batch");
  if (label_smoothing != 0.f)
    hipLaunchKernelGGL(softmax_xent_mix_kernel<true>, dim3(N), dim3(256), 0, st, logits, labels_a, labels_b, lam,
                       dlogits, ws, V, 1.f / (float)N, label_smoothing);
  else
    hipLaunchKernelGGL(softmax_xent_mix_kernel<false>, dim3(N), dim3(256), 0, st, logits, labels_a, labels_b, lam,
                       dlogits, ws, V, 1.f / (float)N, 0.f);
  hipLaunchKernelGGL(mix_mean_kernel, dim3(1), dim3(256), 0, st, ws, N, loss);
}

}  // namespace pdt::mix
