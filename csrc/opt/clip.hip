// Global gradient-norm clipping on the device (torch.nn.utils.clip_grad_norm_'s coefficient) over
// ONE flat fp32 gradient buffer of n elements:
//   sumsq    : fixed chunks of kClipChunk elements, one block per chunk by grid stride; float64 per
//              thread, wave butterfly, 4 waves through LDS; gpart[chunk] = sum g^2 (read-only, 4 B
//              per element);
//   finalize : one block; thread k takes partials k, k + 256, ..., then the same butterfly and LDS
//              step; writes the clip record (norm, coef) of clip.h;
//   scale    : g *= coef in place for the optimizers that cannot read the record (SGD, LARS); the
//              fused LAMB / AdamW pass multiplies as it loads instead (lamb.hip) and skips this pass.
// No floating-point atomics: a chunk's elements, a thread's share of them and every tree are fixed
// by n alone, so the record does not depend on the grid or the stream.  The host never reads it.
#include "kernels/common.h"
#include "opt/clip.h"

#include <algorithm>
#include <stdexcept>

namespace pdt::opt {

// sum over the block's 256 threads in a fixed tree; the result is valid in thread 0
__device__ __forceinline__ double block_sum_f64(double x, double* red) {
  const int t = threadIdx.x;
  x = wave_sum_f64(x);
  if ((t & 63) == 0) red[t >> 6] = x;
  __syncthreads();
  const double s = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();  // red is reused by the next chunk
  return s;
}

__device__ __forceinline__ double sq4(const float4 v, double acc) {
  const double x = v.x, y = v.y, z = v.z, w = v.w;
  acc = fma(x, x, acc);
  acc = fma(y, y, acc);
  acc = fma(z, z, acc);
  return fma(w, w, acc);
}

__global__ void __launch_bounds__(256) clip_sumsq_kernel(const float* __restrict__ g, int64_t n, int nchunks,
                                                         double* __restrict__ gpart) {
  __shared__ double red[4];
  const int t = threadIdx.x;
  for (int c = (int)blockIdx.x; c < nchunks; c += (int)gridDim.x) {
    const int64_t s = (int64_t)c * kClipChunk;
    const int len = (int)min((int64_t)kClipChunk, n - s);
    // g is 16-byte aligned and s a multiple of 4096: every chunk is float4 up to the buffer's tail
    const float4* g4 = reinterpret_cast<const float4*>(g + s);
    double acc = 0.0;
    if (len == kClipChunk) {
      // a whole chunk: the four loads of a thread in flight together, summed in the order of the
      // loop below (vector t, t + 256, t + 512, t + 768)
      const float4 v0 = g4[t], v1 = g4[t + 256], v2 = g4[t + 512], v3 = g4[t + 768];
      acc = sq4(v3, sq4(v2, sq4(v1, sq4(v0, acc))));
    } else {
      const int n4 = len >> 2;
      for (int i = t; i < n4; i += 256) acc = sq4(g4[i], acc);
      for (int i = n4 * 4 + t; i < len; i += 256) {
        const double x = g[s + i];
        acc = fma(x, x, acc);
      }
    }
    const double sum = block_sum_f64(acc, red);
    if (t == 0) gpart[c] = sum;
  }
}

__global__ void __launch_bounds__(256) clip_finalize_kernel(const double* __restrict__ gpart, int nchunks,
                                                            double max_norm, float* __restrict__ clip) {
  __shared__ double red[4];
  double acc = 0.0;
  for (int c = threadIdx.x; c < nchunks; c += 256) acc += gpart[c];
  const double S = block_sum_f64(acc, red);
  if (threadIdx.x == 0) {
    const double norm = sqrt(S);
    const double c = max_norm / (norm + 1e-6);
    clip[kClipNorm] = (float)norm;
    clip[kClipCoef] = (float)(c >= 1.0 ? 1.0 : c);  // a NaN fails the comparison and stays NaN
  }
}

__global__ void __launch_bounds__(256) clip_scale_kernel(float* __restrict__ g, int64_t n,
                                                         const float* __restrict__ clip) {
  const float coef = clip[kClipCoef];
  if (coef == 1.0f) return;  // not clipped: g keeps its bits and its cache lines
  const int64_t n4 = n >> 2;
  float4* g4 = reinterpret_cast<float4*>(g);
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    float4 v = g4[i];
    v.x = coef * v.x; v.y = coef * v.y; v.z = coef * v.z; v.w = coef * v.w;
    g4[i] = v;
  }
  if (blockIdx.x == 0)
    for (int64_t i = n4 * 4 + threadIdx.x; i < n; i += 256) g[i] = coef * g[i];
}

static void check_flat(const void* g, int64_t n, const void* clip) {
  if (!g || !clip || n <= 0) throw std::runtime_error("clip: missing gradient buffer or clip record");
  if (((uintptr_t)g & 15) != 0 || ((uintptr_t)clip & 3) != 0)
    throw std::runtime_error("clip: the gradient buffer must be 16-byte aligned");
}

void launch_grad_norm(const float* g, int64_t n, double* gpart, float* clip, double max_norm, hipStream_t st) {
  check_flat(g, n, clip);
  const int64_t nchunks = clip_chunks(n);
  if (!gpart || ((uintptr_t)gpart & 7) != 0 || nchunks >= (int64_t(1) << 30))
    throw std::runtime_error("clip: missing partials, or too many chunks");
  // one block per chunk up to 65536 blocks, a grid stride beyond (a 2048-block grid measured the
  // same on ResNet-50's 6240 chunks: 24.2 us against 24.0)
  const unsigned grid = (unsigned)std::min<int64_t>(nchunks, 1 << 16);
  hipLaunchKernelGGL(clip_sumsq_kernel, dim3(grid), dim3(256), 0, st, g, n, (int)nchunks, gpart);
  hipLaunchKernelGGL(clip_finalize_kernel, dim3(1), dim3(256), 0, st, gpart, (int)nchunks, max_norm, clip);
}

void launch_scale_grads(float* g, int64_t n, const float* clip, hipStream_t st) {
  check_flat(g, n, clip);
  const int64_t vecs = std::max<int64_t>(n >> 2, 1);
  const unsigned grid = (unsigned)std::min<int64_t>((vecs + 255) / 256, 4096);
  hipLaunchKernelGGL(clip_scale_kernel, dim3(grid), dim3(256), 0, st, g, n, clip);
}

}  // namespace pdt::opt
