// Launcher of the resampling gather (RandomResizedCrop / centre crop + resize), compiled without
// PyTorch headers like csrc/kernels.  It lives in a module of its own (`_C_img`, bind_img.cpp): the
// public surface of `_C` is pinned.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pdt::img {

// largest source or output side: keeps the kernel's integer tap weights inside 32 bits
constexpr int kMaxSide = 16384;

// out[b][c][y][x] = norm(sum over taps of wy * wx * src[idx[b]][c][.][.]), fp32 NCHW [B, C, OH, OW]:
// the box (y0, x0, h, w) of sample idx[b] resized to OH x OW with antialiased bilinear weights
// (data/resize.py), then flipped along x where flip[b], /255 for a uint8 source, (p - mean) / std
// when `normalize`.  box int32 [B][4], 16-byte aligned; flip may be null; N = images in src.
// A box is clamped into the image and idx into [0, N) before anything is read.
void launch_resized_crop(const void* src, bool src_u8, int64_t N, const int64_t* idx, const int32_t* box,
                         const bool* flip, float* out, int B, int C, int H, int W, int OH, int OW, bool normalize,
                         const float* mean, const float* stdv, hipStream_t st);

}  // namespace pdt::img
