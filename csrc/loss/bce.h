// Launcher of the binary cross-entropy loss head, compiled without PyTorch headers like
// csrc/kernels.  It lives in a module of its own (`_C_loss`, bind_loss.cpp): the public surface of
// `_C` is pinned.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pdt::loss {

// Sigmoid cross entropy of logits fp32 [N, C] against the target
//   t_c = lam * T_a(c) + (1 - lam) * T_b(c),  T_x(c) = (c == x) ? on : off,
// (T_a alone where lam is null or a == b), binarised to (t_c > thr) when thr >= 0: the loss
// (sum over all elements times inv_count) and dlogits = (sigmoid(z) - t) * inv_count in one launch.
//   labels_b, lam: both null (hard labels) or both given.
//   row_sums: N doubles, scratch of this call.
//   ticket:   one uint32 that is ZERO on entry; the launch leaves it zero again.
void launch_bce_with_logits(const float* logits, const int64_t* labels_a, const int64_t* labels_b,
                            const float* lam, float* loss, float* dlogits, double* row_sums, uint32_t* ticket,
                            int N, int C, float on, float off, float thr, double inv_count, hipStream_t st);

}  // namespace pdt::loss
