// Binary cross entropy with logits against the smoothed, mixed and optionally thresholded label
// target of the "ResNet strikes back" recipe: every class an independent sigmoid (semantics:
// ops/reference.py::bce_with_logits).  One launch gives the scalar loss and the whole dlogits.
//
// Work split: one wave per row, kRows rows per 256-thread block, the row walked in column tiles of
// kTile vectors per lane (16-byte vectors when C % 4 == 0 and the bases are aligned, single floats
// otherwise), so any C is served.  A tile's logits are loaded first, all of them, and stay in
// registers through the loss term and the gradient store: each logit is read from memory once and
// the kTile loads of a lane are in flight together.  Unlike the softmax heads the gradient of an
// element does not wait for a row statistic, so nothing is staged in LDS.
//
// The target never exists in memory.  A row has at most three distinct target values -- on column
// a, on column b, everywhere else -- and they are formed once per wave, in fp32, by the expression
// of the reference, `lam * T_a + (1 - lam) * T_b` with the two products rounded on their own
// (contraction is OFF for this file), then compared with the threshold.  lam == 1 gives
// 1 * T_a + 0 * T_b = T_a exactly, so that call equals the hard-label call (lam == nullptr) bit for
// bit whatever labels_b holds.
//
// One transcendental pair per element: e = exp(-|z|) feeds both log1p(e) of the loss and the
// sigmoid, (z >= 0 ? 1 : e) / (1 + e).  Element losses are summed in fp64 (a lane's running sum,
// then the fixed butterfly of wave_sum_f64), so the scalar's error is that of its terms.
//
// The scalar loss comes out of the same launch, deterministically and without floating-point
// atomics: lane 0 of a wave stores its row's sum, every wave waits for its store, the block's
// barrier collects the waves, and one lane fences (release), takes a ticket with an ordinary
// integer atomic add and fences again (acquire) -- the hand-off of csrc/img/autoaug.hip.  The block
// that draws the last ticket adds the row sums in a fixed order (lane l takes rows l, l + 64, ...
// ascending, then the same butterfly), writes the loss and puts the ticket back to zero for the
// next launch: no memset in front of the call, nothing a captured graph could not replay.
#include "bce.h"

#include <stdexcept>

#include "kernels/common.h"

#pragma clang fp contract(off)

namespace pdt::loss {

namespace {

constexpr int kThreads = 256;
constexpr int kRows = kThreads / 64;  // one wave per row
constexpr int kTile = 4;              // vectors per lane and column tile

template <int V> struct Vec;
template <> struct Vec<4> { typedef float4 type; };
template <> struct Vec<1> { typedef float type; };

// the reference's blend: both products rounded, then the add
__device__ __forceinline__ float blend(float l, float oml, float ta, float tb) { return l * ta + oml * tb; }

// one element: adds its loss to acc, returns its gradient
__device__ __forceinline__ float bce_elem(float z, float t, float scale, double& acc) {
  const float e = expf(-fabsf(z));
  acc += (double)fmaf(-z, t, fmaxf(z, 0.f)) + (double)log1pf(e);
  const float sig = (z >= 0.f ? 1.f : e) / (1.f + e);
  return (sig - t) * scale;
}

template <int V>
__global__ void __launch_bounds__(kThreads) bce_with_logits_kernel(
    const float* __restrict__ logits, const int64_t* __restrict__ labels_a, const int64_t* __restrict__ labels_b,
    const float* __restrict__ lam, float* __restrict__ loss, float* __restrict__ dlogits,
    double* __restrict__ row_sums, uint32_t* __restrict__ ticket, int N, int C, float on, float off, float thr,
    double inv_count) {
  typedef typename Vec<V>::type vec;
  __shared__ bool is_last;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * kRows + wid;
  if (row < N) {  // wave-uniform: the waves of a partial block past the batch only meet the barrier
    // the row's three target values; a label outside [0, C) matches no column
    const int64_t a64 = labels_a[row];
    const int la = a64 >= 0 && a64 < C ? (int)a64 : -1;
    int lb = la;
    float t_a = on, t_b = off, t_off = off;
    if (lam != nullptr) {
      const int64_t b64 = labels_b[row];
      lb = b64 >= 0 && b64 < C ? (int)b64 : -1;
      if (lb != la) {  // a == b: the row's target is T_a
        const float l = lam[row], oml = 1.f - l;
        t_a = blend(l, oml, on, off);
        t_b = blend(l, oml, off, on);
        t_off = blend(l, oml, off, off);
      }
    }
    if (thr >= 0.f) {
      t_a = t_a > thr ? 1.f : 0.f;
      t_b = t_b > thr ? 1.f : 0.f;
      t_off = t_off > thr ? 1.f : 0.f;
    }
    const float scale = (float)inv_count;
    const float* __restrict__ x = logits + row * C;
    float* __restrict__ g = dlogits + row * C;
    const int nv = C / V;  // V == 4 only when C % 4 == 0
    double acc = 0.0;
    for (int base = 0; base < nv; base += kTile * 64) {
      vec z[kTile];
#pragma unroll
      for (int k = 0; k < kTile; ++k) {
        const int i = base + k * 64 + lane;
        if (i < nv) z[k] = reinterpret_cast<const vec*>(x)[i];
      }
#pragma unroll
      for (int k = 0; k < kTile; ++k) {
        const int i = base + k * 64 + lane;
        if (i >= nv) continue;
        if constexpr (V == 4) {
          const int c = i * 4;
          float4 d;
          d.x = bce_elem(z[k].x, c == la ? t_a : (c == lb ? t_b : t_off), scale, acc);
          d.y = bce_elem(z[k].y, c + 1 == la ? t_a : (c + 1 == lb ? t_b : t_off), scale, acc);
          d.z = bce_elem(z[k].z, c + 2 == la ? t_a : (c + 2 == lb ? t_b : t_off), scale, acc);
          d.w = bce_elem(z[k].w, c + 3 == la ? t_a : (c + 3 == lb ? t_b : t_off), scale, acc);
          reinterpret_cast<float4*>(g)[i] = d;
        } else {
          g[i] = bce_elem(z[k], i == la ? t_a : (i == lb ? t_b : t_off), scale, acc);
        }
      }
    }
    acc = wave_sum_f64(acc);
    if (lane == 0) row_sums[row] = acc;
  }
  // the last block to arrive forms the scalar.  Every wave waits until its own store has been
  // performed, the barrier collects the waves, and one lane fences and takes the ticket for the block
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    is_last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    __threadfence();
  }
  __syncthreads();
  if (!is_last || wid != 0) return;
  double s = 0.0;
  for (int i = lane; i < N; i += 64) s += __hip_atomic_load(row_sums + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  s = wave_sum_f64(s);
  if (lane == 0) {
    loss[0] = (float)(s * inv_count);
    *ticket = 0u;  // every block has drawn: the next launch finds it zero
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

void launch_bce_with_logits(const float* logits, const int64_t* labels_a, const int64_t* labels_b,
                            const float* lam, float* loss, float* dlogits, double* row_sums, uint32_t* ticket,
                            int N, int C, float on, float off, float thr, double inv_count, hipStream_t st) {
  if (N <= 0 || C <= 0) throw std::runtime_error("bce_with_logits: empty logits");
  if ((labels_b == nullptr) != (lam == nullptr))
    throw std::runtime_error("bce_with_logits: labels_b and lam go together");
  const dim3 grid((unsigned)((N + kRows - 1) / kRows));
  if (C % 4 == 0 && aligned16(logits) && aligned16(dlogits))  // then every row base is aligned too
    hipLaunchKernelGGL(bce_with_logits_kernel<4>, grid, dim3(kThreads), 0, st, logits, labels_a, labels_b, lam, loss,
                       dlogits, row_sums, ticket, N, C, on, off, thr, inv_count);
  else
    hipLaunchKernelGGL(bce_with_logits_kernel<1>, grid, dim3(kThreads), 0, st, logits, labels_a, labels_b, lam, loss,
                       dlogits, row_sums, ticket, N, C, on, off, thr, inv_count);
}

}  // namespace pdt::loss
