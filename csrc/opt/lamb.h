// Launchers of the fused LAMB / AdamW step over one flat fp32 parameter space, compiled without
// PyTorch headers like csrc/kernels.  They live in a module of their own (`_C_opt`, bind_opt.cpp):
// the public surface of `_C` is pinned.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels/kernels.h"  // LarsSeg / LarsChunk: the segment / chunk table of optim/lars.py

namespace pdt::opt {

constexpr int kLambChunk = 4096;  // elements a chunk entry may hold (the table's lars_chunk_elems())

// The optimizer's device record.  `done` counts finished updates; the update in flight is number
// t = done + 1.  bc1 / sbc2 are the bias corrections of that update, 1 - beta1^t and
// sqrt(1 - beta2^t), evaluated in float64 and rounded to fp32: the trust launch writes them for the
// update pass, so no launch reads the counter while another block of it advances it.
struct LambRecord {
  int64_t done;
  float bc1, sbc2;
};

struct LambSpace {
  const void* table;   // nseg LarsSeg entries, then nchunks LarsChunk entries (device bytes)
  int nseg, nchunks;
  int64_t numel;       // elements of the flat buffers (chunks outside are skipped)
  double* partials;    // [nchunks][2] = (sum p^2, sum u^2) per chunk
  float* trust;        // [nseg]
  LambRecord* rec;
};

// fp32 flat buffers of one size, 16-byte aligned; `mirror` (or null) receives bf16(p') per element;
// `clip` (or null) is the clip record of clip.h: pass 1 then takes clip[kClipCoef] * g, rounded to
// fp32, for g.  The gradient buffer itself is never written.
struct LambBufs {
  float* p;
  const float* g;
  float* m;
  float* v;
  uint16_t* mirror;
  const float* clip = nullptr;
};

// trust_clip: the ratios of pass 2 are clamped at 1 (timm's Lamb(trust_clip=True))
struct LambHyper {
  double lr, beta1, beta2, eps, wd;
  bool trust_clip = false;
};

// Every launcher covers the segments [seg_lo, seg_hi) and throws std::runtime_error on a range
// outside the table or a misaligned buffer; a chunk entry with n > kLambChunk or a range outside
// the flat buffers is skipped on the device.  max_chunks only sizes the grid.
//
// pass 1: m, v <- moments of update t = done + 1; u = (m / bc1) / (sqrt(v) / sbc2 + eps) + wd_eff p;
// partials[chunk] = (sum p^2, sum u^2) in float64.  A chunk of an excluded segment (wd_eff = 0,
// trust = 1) also gets p -= lr u and its mirror here.
void launch_lamb_moments(const LambBufs& b, const LambSpace& sp, int seg_lo, int seg_hi, int max_chunks,
                         const LambHyper& h, hipStream_t st);
// pass 2: trust[seg] = excluded or |p| == 0 or |u| == 0 ? 1 : float(|p| / |u|); writes the record's
// bias corrections and, with `advance`, done <- done + 1; with h.trust_clip the ratio is min(ratio, 1)
void launch_lamb_trust(const LambSpace& sp, int seg_lo, int seg_hi, const LambHyper& h, bool advance,
                       hipStream_t st);
// pass 3: p -= lr trust[seg] u over the chunks of the segments pass 1 left open (u recomputed from
// the stored moments and the record's bias corrections), and the mirror
void launch_lamb_update(const LambBufs& b, const LambSpace& sp, int seg_lo, int seg_hi, int max_chunks,
                        const LambHyper& h, hipStream_t st);
// the three passes
void launch_lamb(const LambBufs& b, const LambSpace& sp, int seg_lo, int seg_hi, int max_chunks,
                 const LambHyper& h, bool advance, hipStream_t st);
// trust off (AdamW): pass 1's variant that updates every chunk, then (with `advance`) a one-thread
// launch that advances the record.  partials and trust are not touched.
void launch_adamw(const LambBufs& b, const LambSpace& sp, int seg_lo, int seg_hi, int max_chunks,
                  const LambHyper& h, bool advance, hipStream_t st);

}  // namespace pdt::opt
