// Global gradient-norm clipping over one flat fp32 gradient buffer, compiled without PyTorch
// headers like lamb.hip and linked into `_C_opt`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pdt::opt {

constexpr int kClipChunk = 4096;  // elements of one partial: chunk c is [c * 4096, min(n, (c + 1) * 4096))

// The clip record, fp32 [2] on the device: what the optimizer kernels and scale_grads read.
//   [kClipNorm] = float(sqrt(S)), S the float64 sum of squares of the whole buffer
//   [kClipCoef] = float(min(max_norm / (sqrt(S) + 1e-6), 1)), evaluated in float64 and rounded once
//                 (torch.nn.utils.clip_grad_norm_'s coefficient: NaN stays NaN, an infinite norm gives 0)
constexpr int kClipNorm = 0, kClipCoef = 1, kClipRecord = 2;

inline int64_t clip_chunks(int64_t n) { return (n + kClipChunk - 1) / kClipChunk; }

// pass 1: gpart[c] = float64 sum of squares of chunk c, c < clip_chunks(n); pass 2: one block sums
// the partials and writes the record.  Both orders are fixed by n alone (no atomics): the grid and
// the stream never change a bit, and every rank of a data-parallel job gets the same record from
// its copy of the all-reduced gradient.  g must be 16-byte aligned; throws std::runtime_error on a
// null or misaligned operand.
void launch_grad_norm(const float* g, int64_t n, double* gpart, float* clip, double max_norm, hipStream_t st);

// g[i] = clip[kClipCoef] * g[i]; every block returns without touching g when the coefficient is
// exactly 1.0f, so a step that is not clipped costs the launch alone
void launch_scale_grads(float* g, int64_t n, const float* clip, hipStream_t st);

}  // namespace pdt::opt
