// Launcher of the weight-EMA update kernel, compiled without PyTorch headers like csrc/kernels.
// It lives in a module of its own (`_C_ema`, bind_ema.cpp): the public surface of `_C` is pinned.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pdt::ema {

// One fp32 range averaged in place: e <- e + w * (p - e).  `bf`, when set, receives bf16(e') at the
// same element offset (the twin's KRSC weight mirror).
struct LerpSeg {
  float* e = nullptr;
  const float* p = nullptr;
  uint16_t* bf = nullptr;
  int64_t n = 0;
};

// One int64 range copied, not averaged (BatchNorm's num_batches_tracked).
struct CopySeg {
  int64_t* dst = nullptr;
  const int64_t* src = nullptr;
  int64_t n = 0;
};

// The message of the alignment rule a segment breaks, or nullptr: e and p 4-byte aligned and in the
// same 16-byte phase, the bf16 output 8-byte aligned at the first 16-byte-aligned element of e.
const char* lerp_seg_error(const LerpSeg& s);

// ONE launch over the parameter segment, the float-buffer segment and the int64 segment (any of
// them may be empty; nothing is launched when all are).  w = 1 - decay; w == 1 copies p bitwise and
// w == 0 leaves e bitwise unchanged.  Throws std::runtime_error on a segment lerp_seg_error() refuses.
void launch_ema_update(const LerpSeg& params, const LerpSeg& buffers, const CopySeg& counters, float w,
                       hipStream_t st);

}  // namespace pdt::ema
