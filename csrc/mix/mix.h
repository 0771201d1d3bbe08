// Launchers of the batch-mixing kernels (MixUp / CutMix), compiled without PyTorch headers like
// csrc/kernels.  They live in a module of their own (`_C_mix`, bind_mix.cpp): the public surface
// of `_C` is pinned.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pdt::mix {

// launch_augment (csrc/kernels/augment.hip) with per-sample mixing folded into the same pass:
// partner int64 [B] (batch positions), w fp32 [B] (blend weight of the sample itself, 1 = keep),
// box int32 [B][4] = (y1, y2, x1, x2), half-open, in output coordinates.
void launch_augment_mix(const void* src, bool src_u8, const int64_t* idx, const int64_t* oy, const int64_t* ox,
                        const bool* flip, const int64_t* partner, const float* w, const int32_t* box, float* out,
                        int B, int C, int H, int W, int pad, bool normalize, const float* mean, const float* stdv,
                        hipStream_t st);

// softmax cross entropy against the two-label target lam * onehot(a) + (1 - lam) * onehot(b),
// optionally smoothed: loss (mean over rows) and dlogits in one pass.  ws: N floats.
void launch_softmax_xent_mix(const float* logits, const int64_t* labels_a, const int64_t* labels_b,
                             const float* lam, float* loss, float* dlogits, float* ws, int N, int V,
                             hipStream_t st, float label_smoothing);

}  // namespace pdt::mix
