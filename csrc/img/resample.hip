// The ImageNet input transform on the device: augment_kernel (csrc/kernels/augment.hip) with a
// resampling gather.  One pass turns a box of a device-resident source image into a fixed-size
// training or evaluation sample:
//
//   out[b][c][y][x] = norm( sum_jy sum_jx wy[jy] * wx[jx] * src[idx[b]][c][y0 + jy][x0 + jx] )
//
// with ATen's antialiased bilinear weights over the box (y0, x0, h, w) of sample b (semantics and
// oracle: data/resize.py), taps clipped to the box (crop, then resize), the horizontal flip applied
// to the output x, /255 for uint8 sources and (p - mean) / std last.  One thread per four
// consecutive output pixels of a row, one 16-byte store per lane, no LDS.
//
// Weights are formed from integers.  On an axis that maps n source pixels to O output pixels, with
// den = 2 max(n, O) and a = n (2 i + 1) for output position i (the tap centre times 2 O),
//
//   weight of tap j  =  max(0, den - |(2 j + 1) O - a|) / den          (= max(0, 1 - |j + 0.5 - centre| / support))
//   taps             =  [ floor((a - den + O) / 2 O), floor((a + den + O) / 2 O) )  clipped to [0, n)
//
// so the numerators are exact whatever the image size (a tap centre near pixel 200 carries 8e-6 of
// rounding in fp32), and the only roundings are those of the products, the sums and one division by
// the weight total.
//
// A block works on one channel of one sample (grid: plane blocks x C x B), so a wave never mixes
// samples.  Two bodies, chosen per sample and therefore uniform over the wave:
//  * the sample is not down-scaled (h <= OH and w <= OW): the support is one pixel, so an
//    axis has the two taps floor(c) and floor(c) + 1 around c = centre - 0.5 with weights 1 - f and
//    f (they sum to den exactly).  2 x 2 loads per pixel, no loop, no branch; a tap that falls off
//    the box is folded onto the edge pixel with weight 0.  A box of the output's own size has
//    f == 0 everywhere, and the body then returns the source pixel bit for bit.
//  * otherwise: tap loops with run-time bounds, any down-scale factor.  Row weights are formed once
//    per thread and row tap, column weights per pixel; the weight totals are summed as integers.
// A sample's result depends on nothing but its own operands: it is the same bit for bit in any batch.
//
// Floating-point contraction is OFF for this file: the tail p * (1/255), (p - mean) / std rounds
// each operation on its own, as augment_kernel does (its product and difference sit on two sides of
// a branch), so that a box of the output's size reproduces that kernel.  The multiply-adds of the
// tap sums are written out as fmaf.
#include "resample.h"

#include <stdexcept>

#pragma clang fp contract(off)

namespace pdt::img {

namespace {

// floor(a / b) for b > 0: the quotient estimated in fp32 (rb = 1 / b) and corrected by the exact
// remainder.  |a / b| stays below 2^16 here (sides <= kMaxSide), so the estimate is off by one at most.
__device__ __forceinline__ int floor_div(int a, int b, float rb) {
  const int q = (int)floorf((float)a * rb);
  const int r = a - q * b;
  return q + (r >= b ? 1 : 0) - (r < 0 ? 1 : 0);
}

template <bool U8>
__device__ __forceinline__ float load_px(const void* __restrict__ src_, int64_t o) {
  if constexpr (U8) return (float)reinterpret_cast<const uint8_t*>(src_)[o];
  else return reinterpret_cast<const float*>(src_)[o];
}

// the two taps of an axis that is not down-scaled (n <= O), already folded into [0, n)
struct Tap2 {
  int j0, j1;
  float w0, w1;
};

__device__ __forceinline__ Tap2 taps2(int i, int n, int O, float rb) {
  const int b = 2 * O;
  const int a = n * (2 * i + 1) - O;  // (centre - 0.5) * 2 O
  const int j = floor_div(a, b, rb);  // -1 .. n - 1
  const float f = (float)(a - j * b) * rb;  // weight of tap j + 1, in [0, 1)
  Tap2 t;
  t.j0 = min(max(j, 0), n - 1);
  t.j1 = min(max(j + 1, 0), n - 1);
  t.w1 = j < 0 ? 1.f : (j + 1 >= n ? 0.f : f);
  t.w0 = 1.f - t.w1;
  return t;
}

// the taps [lo, hi) of any axis and what their integer weights are formed from
struct Span {
  int lo, hi, a, den;
};

__device__ __forceinline__ Span span(int i, int n, int O, float rb) {
  Span s;
  s.den = 2 * max(n, O);
  s.a = n * (2 * i + 1);
  s.lo = max(floor_div(s.a - s.den + O, 2 * O, rb), 0);
  s.hi = min(floor_div(s.a + s.den + O, 2 * O, rb), n);
  return s;
}

__device__ __forceinline__ int tap_weight(const Span& s, int j, int O) {
  return max(s.den - abs((2 * j + 1) * O - s.a), 0);
}

__device__ __forceinline__ int weight_total(const Span& s, int O) {
  int t = 0;
  for (int j = s.lo; j < s.hi; ++j) t += tap_weight(s, j, O);
  return max(t, 1);  // the tap nearest the centre always weighs den / 2 or more
}

}  // namespace

template <bool U8, bool NORM>
__global__ void __launch_bounds__(256) resized_crop_kernel(
    const void* __restrict__ src_, int64_t N, const int64_t* __restrict__ idx, const int32_t* __restrict__ box,
    const bool* __restrict__ flip, float* __restrict__ out, int C, int H, int W, int OH, int OW, float m0,
    float m1, float m2, float s0, float s1, float s2) {
  // grid (blocks of one output plane, C, B): the sample and the channel are the same for a whole
  // block, so what is read per sample below sits in scalar registers and the choice between the
  // two bodies is uniform
  const int W4 = OW / 4;
  const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);  // position in the plane, 4 pixels each
  if (p >= OH * W4) return;
  const int x4 = p % W4, y = p / W4;
  const int c = (int)blockIdx.y, b = (int)blockIdx.z;
  const int64_t t = ((int64_t)b * C + c) * OH * W4 + p;
  const float mean = c == 0 ? m0 : (c == 1 ? m1 : m2);
  const float stdv = c == 0 ? s0 : (c == 1 ? s1 : s2);
  // the sample's image and box, both forced inside the source before any address is formed
  const int64_t ni = idx[b];
  const int64_t n = ni < 0 ? 0 : (ni >= N ? N - 1 : ni);
  const int4 bx = reinterpret_cast<const int4*>(box)[b];  // y0, x0, h, w
  const int by0 = min(max(bx.x, 0), H - 1);
  const int bx0 = min(max(bx.y, 0), W - 1);
  const int bh = min(max(bx.z, 1), H - by0);
  const int bw = min(max(bx.w, 1), W - bx0);
  const bool fl = flip != nullptr && flip[b];
  const int64_t base = ((n * C + c) * H + by0) * (int64_t)W + bx0;  // the box's first pixel
  const float rby = 1.f / (float)(2 * OH), rbx = 1.f / (float)(2 * OW);
  float v[4];
  if (bh <= OH && bw <= OW) {
    const Tap2 ty = taps2(y, bh, OH, rby);
    const int64_t row0 = base + (int64_t)ty.j0 * W, row1 = base + (int64_t)ty.j1 * W;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int x = x4 * 4 + q;
      const Tap2 tx = taps2(fl ? OW - 1 - x : x, bw, OW, rbx);
      const float p00 = load_px<U8>(src_, row0 + tx.j0), p01 = load_px<U8>(src_, row0 + tx.j1);
      const float p10 = load_px<U8>(src_, row1 + tx.j0), p11 = load_px<U8>(src_, row1 + tx.j1);
      const float top = fmaf(tx.w1, p01, tx.w0 * p00), bot = fmaf(tx.w1, p11, tx.w0 * p10);
      v[q] = fmaf(ty.w1, bot, ty.w0 * top);
    }
  } else {
    const Span sy = span(y, bh, OH, rby);
    Span sx[4];
    float scale[4], acc[4];
    const float ty = (float)weight_total(sy, OH);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int x = x4 * 4 + q;
      sx[q] = span(fl ? OW - 1 - x : x, bw, OW, rbx);
      scale[q] = ty * (float)weight_total(sx[q], OW);
      acc[q] = 0.f;
    }
    for (int jy = sy.lo; jy < sy.hi; ++jy) {
      const float wy = (float)tap_weight(sy, jy, OH);
      const int64_t row = base + (int64_t)jy * W;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float rs = 0.f;
        for (int jx = sx[q].lo; jx < sx[q].hi; ++jx)
          rs = fmaf((float)tap_weight(sx[q], jx, OW), load_px<U8>(src_, row + jx), rs);
        acc[q] = fmaf(wy, rs, acc[q]);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = acc[q] / scale[q];
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float p = v[q];
    if constexpr (U8) p *= 1.0f / 255.0f;
    if constexpr (NORM) p = (p - mean) / stdv;
    v[q] = p;
  }
  *reinterpret_cast<float4*>(out + t * 4) = make_float4(v[0], v[1], v[2], v[3]);
}

void launch_resized_crop(const void* src, bool src_u8, int64_t N, const int64_t* idx, const int32_t* box,
                         const bool* flip, float* out, int B, int C, int H, int W, int OH, int OW, bool normalize,
                         const float* mean, const float* stdv, hipStream_t st) {
  if (OW % 4 != 0) throw std::runtime_error("resized_crop: output width must be a multiple of 4");
  if (C > 3) throw std::runtime_error("resized_crop: at most 3 channels");
  if (N < 1 || H < 1 || W < 1 || OH < 1 || OW < 1 || H > kMaxSide || W > kMaxSide || OH > kMaxSide || OW > kMaxSide)
    throw std::runtime_error("resized_crop: source and output sides must be in [1, 16384]");
  if (B > 65535) throw std::runtime_error("resized_crop: at most 65535 samples per launch");
  if (B <= 0 || C <= 0) return;
  const dim3 grid((unsigned)((OH * (OW / 4) + 255) / 256), (unsigned)C, (unsigned)B);
#define PDT_RRC(U8, NRM)                                                                                 \
  hipLaunchKernelGGL((resized_crop_kernel<U8, NRM>), grid, dim3(256), 0, st, src, N, idx, box, flip, out, C, H, \
                     W, OH, OW, mean[0], mean[1], mean[2], stdv[0], stdv[1], stdv[2])
  if (src_u8) { if (normalize) PDT_RRC(true, true); else PDT_RRC(true, false); }
  else { if (normalize) PDT_RRC(false, true); else PDT_RRC(false, false); }
#undef PDT_RRC
}

}  // namespace pdt::img
