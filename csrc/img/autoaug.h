// Launcher of the fused augmentation policy (TrivialAugmentWide + RandomErasing), compiled without
// PyTorch headers like csrc/kernels.  Bound in `_C_img` (bind_img.cpp); semantics and oracle:
// data/autoaug.py.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace pdt::img {

// largest side: keeps the integer statistics (255 * H * W gray sum, histogram counts) inside 32 bits
constexpr int kAugMaxSide = 4096;
constexpr int kAugOps = 14;

// Per-sample statistics words (uint32): histogram [3][256], gray sum, 255 - min [3], max [3], the
// arrival ticket.  A multiple of 16 bytes, so the block that is zeroed every call stays aligned.
constexpr int kAugStatWords = 3 * 256 + 8;
constexpr int kAugLutBytes = 3 * 256;

// bytes of the workspace of a B-sample call: the statistics block (zeroed by the launcher), then the
// per-sample 3 x 256 uint8 look-up tables
inline size_t autoaug_workspace_bytes(int B) {
  return (size_t)B * (kAugStatWords * sizeof(uint32_t) + kAugLutBytes);
}

// out[b] = erase(norm(policy_b(quantize(x[b])))), fp32 [B, 3, H, W] (W % 4 == 0, sides <= kAugMaxSide):
// x in [0, 1] is quantised to 8-bit levels, sample b goes through operation op[b] (0..13, anything
// else is Identity) with param[b][2] and the inverse matrix matrix[b][6], levels return to [0, 1],
// are normalised with (p - mean) / std when `normalize`, and the box erase[b] = (y0, x0, h, w),
// clamped into the image, is set to 0.  Two launches: a statistics pass (Contrast, AutoContrast and
// Equalize samples only) into `workspace`, and the apply pass.  x, out, erase and workspace: 16-byte
// aligned.  `passes`: bit 0 the statistics pass, bit 1 the apply pass (3 = the op; the apply pass alone
// serves a batch whose operations are all Identity, erasing alone, and either pass alone a timing).
void launch_autoaug(const float* x, const int32_t* op, const float* param, const float* matrix,
                    const int32_t* erase, float* out, void* workspace, int B, int H, int W, bool normalize,
                    const float* mean, const float* stdv, int passes, hipStream_t st);

}  // namespace pdt::img
