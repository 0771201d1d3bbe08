// TrivialAugmentWide + RandomErasing on the device: every sample of a batch goes through its own
// operation (one of 14, drawn by data/autoaug.py, which is also the oracle), then normalisation and
// its erase box, in two launches:
//
//   statistics pass   only for samples whose operation needs the whole image: Contrast (integer sum
//                     of the gray levels), AutoContrast (per-channel min and max) and Equalize
//                     (per-channel 256-bin histogram, built in LDS and merged across the sample's
//                     blocks with integer global atomics: integers make the result independent of
//                     the order).  Every other block leaves on a block-uniform branch.  The last
//                     block of an AutoContrast / Equalize sample to arrive turns the merged
//                     statistics into a 3 x 256 uint8 look-up table.
//   apply pass        out = erase(norm(op(quantize(x)))).  A block owns a tile of one sample, all
//                     three channels (Color needs the pixel's RGB); a lane owns four pixels of a row:
//                     16-byte loads and stores.  The sample's operation, parameters, matrix and box
//                     are uniform loads, so the switch over the operation is uniform over the block.
//
// The input is the fp32 [0, 1] batch of the crop kernels; q = clamp(rint(x * 255), 0, 255) on load.
// Geometric operations gather the fp32 input at the computed index and quantise it; Sharpness reads
// the 3 x 3 neighbourhood of the same channel.
//
// Floating-point contraction is OFF for this file: the oracle defines the blends, the gray level and
// the source coordinates as single rounded fp32 operations in a written order, and a fused
// multiply-add would round once where it rounds twice.
//
// Hand-off inside the statistics pass: every block publishes through agent-scope atomics only; each
// wave drains them, and behind the block's barrier one lane fences (release), takes a ticket with an
// atomic add and fences again (acquire); the block that draws the last ticket reads the merged words
// with agent-scope atomic loads.  Nothing spins.  The statistics block of the workspace is zeroed by a
// memset node in front of every call.
#include "autoaug.h"

#include <stdexcept>
#include <string>

#pragma clang fp contract(off)

namespace pdt::img {

namespace {

enum : int {
  kIdentity = 0, kShearX, kShearY, kTranslateX, kTranslateY, kRotate, kBrightness, kColor, kContrast,
  kSharpness, kPosterize, kSolarize, kAutoContrast, kEqualize
};

constexpr int kThreads = 256;
// pixel quads per thread of the statistics pass: a block covers 4096 pixels of a plane, so a 224 x 224
// sample merges 13 partial histograms, not 49
constexpr int kStatQuads = 4;
// words of a sample's statistics
constexpr int kGraySum = 3 * 256, kMinInv = kGraySum + 1, kMax = kMinInv + 3, kTicket = kMax + 3;
static_assert(kTicket + 1 == kAugStatWords, "statistics layout");

__device__ __forceinline__ float quant(float x) { return fminf(fmaxf(rintf(x * 255.f), 0.f), 255.f); }

__device__ __forceinline__ float gray_level(float r, float g, float b) {
  return truncf((0.2989f * r + 0.587f * g) + 0.114f * b);
}

__device__ __forceinline__ float blend(float a, float b, float r, float r1) {
  return truncf(fminf(fmaxf(r * a + r1 * b, 0.f), 255.f));
}

__device__ __forceinline__ uint32_t load_agent(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool MAX>
__device__ __forceinline__ uint32_t wave_reduce(uint32_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint32_t u = (uint32_t)__shfl_xor((int)v, o, 64);
    v = MAX ? max(v, u) : v + u;
  }
  return v;
}

}  // namespace

// grid (blocks of kThreads * kStatQuads pixel quads, B)
__global__ void __launch_bounds__(kThreads) autoaug_stats_kernel(const float* __restrict__ x,
                                                                 const int32_t* __restrict__ opv,
                                                                 uint32_t* __restrict__ stats,
                                                                 uint8_t* __restrict__ lut, int H, int W) {
  const int b = (int)blockIdx.y;
  const int op = opv[b];
  if (op != kContrast && op != kAutoContrast && op != kEqualize) return;  // uniform over the block
  __shared__ uint32_t hist[3 * 256];
  __shared__ uint32_t part[kThreads / 64][7];
  __shared__ bool is_last;
  const int tid = (int)threadIdx.x;
  const int Q = H * (W / 4);
  const int64_t plane = (int64_t)H * W;
  const float* xs = x + (int64_t)b * 3 * plane;
  uint32_t* ws = stats + (int64_t)b * kAugStatWords;
  if (op == kEqualize) {
    for (int i = tid; i < 3 * 256; i += kThreads) hist[i] = 0u;
    __syncthreads();
  }
  // r[0]: gray sum; r[1..3]: 255 - min per channel; r[4..6]: max per channel
  uint32_t r[7] = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
  // every load of the thread is issued before the first level is used: one memory latency, not four
  float4 v[kStatQuads][3];
#pragma unroll
  for (int k = 0; k < kStatQuads; ++k) {
    const int p = ((int)blockIdx.x * kStatQuads + k) * kThreads + tid;
#pragma unroll
    for (int c = 0; c < 3; ++c)
      v[k][c] = p < Q ? *reinterpret_cast<const float4*>(xs + c * plane + (int64_t)p * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
#pragma unroll
  for (int k = 0; k < kStatQuads; ++k) {
    const int p = ((int)blockIdx.x * kStatQuads + k) * kThreads + tid;
    if (p >= Q) break;
    float q[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      q[c][0] = quant(v[k][c].x); q[c][1] = quant(v[k][c].y); q[c][2] = quant(v[k][c].z); q[c][3] = quant(v[k][c].w);
    }
    if (op == kContrast) {
#pragma unroll
      for (int j = 0; j < 4; ++j) r[0] += (uint32_t)gray_level(q[0][j], q[1][j], q[2][j]);
    } else if (op == kAutoContrast) {
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t v = (uint32_t)q[c][j];
          r[1 + c] = max(r[1 + c], 255u - v);
          r[4 + c] = max(r[4 + c], v);
        }
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) atomicAdd(&hist[c * 256 + (int)q[c][j]], 1u);
    }
  }
  if (op == kEqualize) {
    __syncthreads();
    for (int i = tid; i < 3 * 256; i += kThreads)
      if (hist[i] != 0u) atomicAdd(&ws[i], hist[i]);
  } else {
    const int first = op == kContrast ? 0 : 1, last = op == kContrast ? 1 : 7;
    for (int i = first; i < last; ++i) {
      const uint32_t v = i == 0 ? wave_reduce<false>(r[i]) : wave_reduce<true>(r[i]);
      if ((tid & 63) == 0) part[tid >> 6][i] = v;
    }
    __syncthreads();
    if (tid >= first && tid < last) {
      uint32_t v = part[0][tid];
      for (int w = 1; w < kThreads / 64; ++w) v = tid == 0 ? v + part[w][tid] : max(v, part[w][tid]);
      if (tid == 0) atomicAdd(&ws[kGraySum], v);
      else atomicMax(&ws[kGraySum + tid], v);
    }
    if (op == kContrast) return;  // the apply pass forms the mean itself
  }
  // the last block of the sample to arrive builds the table.  Every wave waits until its own atomics
  // have been performed, the barrier collects the waves, and one lane fences and takes the ticket for
  // the block: an agent-scope fence writes the L2 back, so it is issued once per block, not per wave
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    __threadfence();
    is_last = atomicAdd(&ws[kTicket], 1u) == gridDim.x - 1;
    __threadfence();
  }
  __syncthreads();
  if (!is_last) return;
  uint8_t* l = lut + (int64_t)b * kAugLutBytes;
  if (op == kAutoContrast) {
    for (int c = 0; c < 3; ++c) {
      const uint32_t lo = 255u - load_agent(&ws[kMinInv + c]), hi = load_agent(&ws[kMax + c]);
      float v = (float)tid;
      if (hi > lo) {
        const float scale = __fdiv_rn(255.f, (float)(hi - lo));
        v = truncf(fminf(fmaxf(((float)tid - (float)lo) * scale, 0.f), 255.f));
      }
      l[c * 256 + tid] = (uint8_t)v;
    }
    return;
  }
  for (int i = tid; i < 3 * 256; i += kThreads) hist[i] = load_agent(&ws[i]);
  __syncthreads();
  for (int c = 0; c < 3; ++c) {
    uint32_t below = 0u, last_bin = 0u;  // pixels under level tid; the count of the last level in use
    for (int i = 0; i < 256; ++i) {
      const uint32_t h = hist[c * 256 + i];
      if (i < tid) below += h;
      if (h != 0u) last_bin = h;
    }
    const uint32_t step = ((uint32_t)(H * W) - last_bin) / 255u;
    uint32_t v = (uint32_t)tid;
    if (step != 0u) v = tid == 0 ? 0u : min(255u, (below + step / 2u) / step);
    l[c * 256 + tid] = (uint8_t)v;
  }
}

// grid (blocks of kThreads pixel quads, B)
template <bool NORM>
__global__ void __launch_bounds__(kThreads) autoaug_apply_kernel(
    const float* __restrict__ x, const int32_t* __restrict__ opv, const float* __restrict__ param,
    const float* __restrict__ matrix, const int32_t* __restrict__ erase, const uint32_t* __restrict__ stats,
    const uint8_t* __restrict__ lut, float* __restrict__ out, int H, int W, float mean0, float mean1,
    float mean2, float std0, float std1, float std2) {
  // everything read per sample below is the same for the whole block: scalar registers
  const int b = (int)blockIdx.y;
  int op = opv[b];
  if ((unsigned)op >= (unsigned)kAugOps) op = kIdentity;
  if (op == kSharpness && (H <= 2 || W <= 2)) op = kIdentity;
  const float p0 = param[2 * b], p1 = param[2 * b + 1];
  const int4 bx = reinterpret_cast<const int4*>(erase)[b];  // y0, x0, h, w, clamped into the image
  const int ey0 = min(max(bx.x, 0), H), ex0 = min(max(bx.y, 0), W);
  const int ey1 = ey0 + min(max(bx.z, 0), H - ey0), ex1 = ex0 + min(max(bx.w, 0), W - ex0);
  const int tid = (int)threadIdx.x;
  __shared__ uint32_t lut_s[kAugLutBytes / 4];
  if (op == kAutoContrast || op == kEqualize) {
    if (tid < kAugLutBytes / 4)
      lut_s[tid] = reinterpret_cast<const uint32_t*>(lut + (int64_t)b * kAugLutBytes)[tid];
    __syncthreads();
  }
  const int W4 = W / 4;
  const int p = (int)blockIdx.x * kThreads + tid;  // position in the plane, 4 pixels each
  if (p >= H * W4) return;
  const int y = p / W4, x0 = (p % W4) * 4;
  const int64_t plane = (int64_t)H * W;
  const float* xs = x + (int64_t)b * 3 * plane;
  float lv[3][4];  // the levels after the operation
  if (op >= kShearX && op <= kRotate) {
    const float* m = matrix + 6 * b;
    const float m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5];
    const float hw = (float)W * 0.5f, hh = (float)H * 0.5f;
    const float yc = ((float)y + 0.5f) - hh;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float xc = ((float)(x0 + j) + 0.5f) - hw;
      const float sx = ((m0 * xc + m1 * yc) + m2) + (hw - 0.5f);
      const float sy = ((m3 * xc + m4 * yc) + m5) + (hh - 0.5f);
      const float fx = rintf(sx), fy = rintf(sy);
      // a NaN coordinate fails every comparison: outside
      const bool inside = fx >= 0.f && fx <= (float)(W - 1) && fy >= 0.f && fy <= (float)(H - 1);
      const int o = inside ? (int)fy * W + (int)fx : 0;
#pragma unroll
      for (int c = 0; c < 3; ++c) lv[c][j] = inside ? quant(xs[c * plane + o]) : 0.f;
    }
  } else if (op == kSharpness) {
    const int ym = max(y - 1, 0), yp = min(y + 1, H - 1);
    const int xl = max(x0 - 1, 0), xr = min(x0 + 4, W - 1);
    const bool row_in = y >= 1 && y <= H - 2;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float t[3][6];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float* row = xs + c * plane + (int64_t)(k == 0 ? ym : (k == 1 ? y : yp)) * W;
        const float4 v = *reinterpret_cast<const float4*>(row + x0);
        t[k][0] = quant(row[xl]);
        t[k][1] = quant(v.x); t[k][2] = quant(v.y); t[k][3] = quant(v.z); t[k][4] = quant(v.w);
        t[k][5] = quant(row[xr]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float q = t[1][j + 1];
        float blur = q;  // border pixels keep their level
        if (row_in && x0 + j >= 1 && x0 + j <= W - 2) {
          int s = 4 * (int)q;
#pragma unroll
          for (int k = 0; k < 3; ++k) s += (int)t[k][j] + (int)t[k][j + 1] + (int)t[k][j + 2];
          blur = (float)((2 * s + 13) / 26);
        }
        lv[c][j] = blend(q, blur, p0, p1);
      }
    }
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float4 v = *reinterpret_cast<const float4*>(xs + c * plane + (int64_t)p * 4);
      lv[c][0] = quant(v.x); lv[c][1] = quant(v.y); lv[c][2] = quant(v.z); lv[c][3] = quant(v.w);
    }
    if (op == kBrightness || op == kColor || op == kContrast) {
      float other = 0.f;
      if (op == kContrast)
        other = __fdiv_rn((float)stats[(int64_t)b * kAugStatWords + kGraySum], (float)(H * W));
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (op == kColor) other = gray_level(lv[0][j], lv[1][j], lv[2][j]);
#pragma unroll
        for (int c = 0; c < 3; ++c) lv[c][j] = blend(lv[c][j], other, p0, p1);
      }
    } else if (op == kPosterize) {
      const int bits = min(max((int)p0, 0), 8);
      const int mask = (0xFF << (8 - bits)) & 0xFF;
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) lv[c][j] = (float)((int)lv[c][j] & mask);
    } else if (op == kSolarize) {
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) lv[c][j] = lv[c][j] >= p0 ? 255.f - lv[c][j] : lv[c][j];
    } else if (op == kAutoContrast || op == kEqualize) {
      const uint8_t* ls = reinterpret_cast<const uint8_t*>(lut_s);
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) lv[c][j] = (float)ls[c * 256 + (int)lv[c][j]];
    }
  }
  const bool row_erased = y >= ey0 && y < ey1;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float mean = c == 0 ? mean0 : (c == 1 ? mean1 : mean2);
    const float stdv = c == 0 ? std0 : (c == 1 ? std1 : std2);
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float q = lv[c][j] * (1.0f / 255.0f);
      if constexpr (NORM) q = (q - mean) / stdv;
      v[j] = row_erased && x0 + j >= ex0 && x0 + j < ex1 ? 0.f : q;
    }
    *reinterpret_cast<float4*>(out + ((int64_t)b * 3 + c) * plane + (int64_t)p * 4) =
        make_float4(v[0], v[1], v[2], v[3]);
  }
}

void launch_autoaug(const float* x, const int32_t* op, const float* param, const float* matrix,
                    const int32_t* erase, float* out, void* workspace, int B, int H, int W, bool normalize,
                    const float* mean, const float* stdv, int passes, hipStream_t st) {
  if (W % 4 != 0) throw std::runtime_error("autoaug: width must be a multiple of 4");
  if (H < 1 || W < 1 || H > kAugMaxSide || W > kAugMaxSide)
    throw std::runtime_error("autoaug: sides must be in [1, 4096]");
  if (B > 65535) throw std::runtime_error("autoaug: at most 65535 samples per launch");
  if (B <= 0) return;
  uint32_t* stats = reinterpret_cast<uint32_t*>(workspace);
  uint8_t* lut = reinterpret_cast<uint8_t*>(workspace) + (size_t)B * kAugStatWords * sizeof(uint32_t);
  const int Q = H * (W / 4);
  if (passes & 1) {
    if (hipMemsetAsync(stats, 0, (size_t)B * kAugStatWords * sizeof(uint32_t), st) != hipSuccess)
      throw std::runtime_error("autoaug: clearing the statistics failed");
    const dim3 grid((unsigned)((Q + kThreads * kStatQuads - 1) / (kThreads * kStatQuads)), (unsigned)B);
    hipLaunchKernelGGL(autoaug_stats_kernel, grid, dim3(kThreads), 0, st, x, op, stats, lut, H, W);
  }
  if (passes & 2) {
    const dim3 grid((unsigned)((Q + kThreads - 1) / kThreads), (unsigned)B);
#define PDT_AUG_APPLY(NRM)                                                                                    \
  hipLaunchKernelGGL((autoaug_apply_kernel<NRM>), grid, dim3(kThreads), 0, st, x, op, param, matrix, erase, \
                     stats, lut, out, H, W, mean[0], mean[1], mean[2], stdv[0], stdv[1], stdv[2])
    if (normalize) PDT_AUG_APPLY(true); else PDT_AUG_APPLY(false);
#undef PDT_AUG_APPLY
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) throw std::runtime_error(std::string("autoaug: launch failed: ") + hipGetErrorString(e));
}

}  // namespace pdt::img
