// Implicit-GEMM convolution for gfx950 (MI355X / CDNA4): forward, data-gradient
// and weight-gradient, NHWC bf16 in, fp32 MFMA accumulation.
//
// Why implicit GEMM on MFMA: every ResNet conv is GEMM-shaped
// (SURVEY.md §2.6): fwd M=N*Ho*Wo, N=K, K=R*S*C; dgrad M=N*H*W, N=C,
// K=K*R*S; wgrad M=K, N=R*S*C, K=N*Ho*Wo.  The im2col matrix is never
// materialised: the A-tile loader gathers 16-byte (8-channel) NHWC vectors
// straight from the activation with bounds-checked buffer loads (padding reads
// return 0 from the buffer unit's range check -- no branches, no zero fill),
// stages them in LDS with an XOR swizzle that makes the MFMA fragment reads
// bank-conflict free, and the waves run v_mfma_f32_16x16x32_bf16.
//
// Kernel families
//   igemm_nt : A rows k-contiguous (gathered activations), B rows k-contiguous
//              (packed weights).  fwd: B = W[K][R][S][C].  dgrad: A = dy,
//              B = W^T[C][R][S][K]; stride > 1 is split into stride^2 parity
//              classes (one launch each) so no MFMA work is spent on the
//              structural zeros of the transposed convolution.  The fwd
//              epilogue also emits BatchNorm partial statistics (sum and M2 per
//              workgroup row tile per channel) from the fp32 accumulators, so BN
//              never re-reads the conv output to compute its batch stats.
//   igemm_tn : wgrad.  Both operands have the reduction index (pixels) as the
//              strided dimension, so tiles are staged [m][col] and fragments are
//              read with the CDNA4 transposing LDS read ds_read_b64_tr_b16.
//              Long reductions (up to 3.2M pixels) are split-K over blockIdx.z
//              into an fp32 slab reduced by a second deterministic pass.
//
// Pipeline (both): 4 waves, BK = 64, two LDS buffers, register-staged prefetch
// of tile k+1 issued before the MFMAs of tile k and written to LDS after them,
// one barrier per K-step.  Block ids are remapped so consecutive tiles (sharing
// the A panel) run on the same XCD and hit its L2.
#include "common.h"
#include "igemm_common.h"
#include "kernels.h"

#include <algorithm>
#include <stdexcept>
#include <string>
#include <type_traits>

namespace pdt {


// Operand element type of the NT kernel: bf16, or fp8 with the activation operand in e4m3
// (forward) or e5m2 (gradients); weights are always e4m3.  A K-step moves 128 bytes of every
// operand row either way: 64 bf16 (two 16x16x32 MFMAs) or 128 fp8 (one MX-rate 16x16x128 MFMA,
// twice the bf16 FLOP per cycle).  Offsets below are element offsets scaled by EB bytes.
constexpr int OP_BF16 = 0;
constexpr int OP_F8_E4M3 = 1;
constexpr int OP_F8_E5M2 = 2;

typedef int v8i __attribute__((ext_vector_type(8)));

// D += W(16 x 128, e4m3) * X(128 x 16, fmt XF), unit E8M0 block scales (the literal 0 operands
// select the unscaled encoding: tests/test_fp8_gpu.py).  Lane l: row/col l&15, k bytes
// 32*(l>>4) .. +31 -- identical for both operands, which is all the product needs.
template <int XF>
__device__ __forceinline__ v4f mfma_f8(const v8i& w, const v8i& x, const v4f& c) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, x, c, 0, XF == OP_F8_E5M2 ? 1 : 0, 0, 0, 0, 0);
}

// ============================================================================
//                          NT implicit GEMM (fwd / dgrad)
// ============================================================================
struct NtArgs {
  const uint16_t* a;   // activation source NHWC (x for fwd, dy for dgrad), CA channels
  const uint16_t* b;   // [Nout][Kg] k-contiguous
  uint16_t* out;       // NHWC output, Nout channels
  const uint16_t* addend;  // optional NHWC tensor (same layout as out) added in the epilogue
  float* part;         // BN partials [ngroups][2][Nout] or null
  const float* oscale; // fp8 operands: per-output-column dequantization factor (acc * oscale[col])
  const float* ascale; // fp8 operands: activation dequantization factor (device scalar) or null
  uint32_t a_bytes, b_bytes;
  uint32_t o_bytes;    // bytes of the output tensor (= of addend / bn_y / bn_z, same layout)
  int HA, WA, CA;      // A source dims
  int Nout, Kg, S;     // GEMM N, B row length (= taps_total*CA), filter width (generic path)
  int M;               // GEMM rows of this launch
  FastDiv div_ij, div_j;  // m -> n = m / Mij, i = rem / Mj
  FastDiv div_ca, div_s;  // generic (non-C64) loader: k -> tap = k / CA, tap -> r = tap / S
  int Mij, Mj;
  int ash, asw, aoff_h, aoff_w;     // A base coords: h0 = i*ash + aoff_h
  int OH, OW, osh, osw, oph, opw;   // out row = (n*OH + i*osh + oph)*OW + j*osw + opw
  int dense;           // output row == m (no scatter)
  // taps of this launch form a grid (i < tnr, j < tns): filter tap (tr0 + i*tstep, ts0 + j*tstep),
  // A-coordinate offset (dr0 + i*dstep, ds0 + j*dstep).  Closed form -> pure scalar math in the
  // K loop (a per-tap table in kernel args would be read with vector loads every K-step).
  int ntaps, tnr, tns, tr0, ts0, tstep, dr0, ds0, dstep;
  int c8, c8_rows, c8_step;  // generic loader, 8-channel source with S | 8: rows / bytes per K-step
  // EPI_BNB (dgrad): BN-backward of the unit that produced this conv's input, fused into the
  // epilogue.  out = g = dx * relu'(unit) and per-(workgroup row tile, channel) partials of
  // (sum g, sum g*(y - mean)) go to bn_part[bn_group0 + row_tile][2][Nout].
  const uint16_t* bn_y;   // that unit's pre-BN conv output (same layout as out)
  const uint16_t* bn_z;   // its post-activation output (mask mode 1 only), or for mask mode 3 its
                          // ReLU bitmask: one byte per 8-channel chunk, bit q = (z[c0 + q] > 0)
  const float* bn_stats;  // [4][Nout] mean, invstd, scale, shift
  float* bn_part;
  // second BatchNorm on the SAME gradient g (acc mode, mask 3 + addend only): a downsampling block's
  // projection-shortcut BN, whose input gradient is that block's output gradient too.  Its y and
  // mean, and an fp32 [2][Nout] accumulator of (sum g, sum g*(y2 - mean2)) -- the reduction pass the
  // shortcut's BN backward would otherwise run over g and y2
  const uint16_t* bn_y2;
  const float* bn_stats2;
  float* bn_acc2;
  float* bn_acc;  // non-null: fp32-atomic accumulation of the partials into [2][Nout] instead
  int bn_mask, bn_group0;
  // addend layout: 0 = same NHWC layout as out; 2 = compact stride-2 map addend[n][h/2][w/2] that
  // contributes only at even (h, w) -- the input gradient of a 1x1/s2 projection shortcut, which
  // is zero at every odd position and is never materialised at full resolution
  int add_sub, add_h, add_w;
  uint32_t add_bytes;  // bytes of the addend tensor
  // HALO (3x3, stride 1, same-size output): the A tile of a channel block is staged ONCE as the
  // halo of the tile's image rows -- halo_rows x (WA + 2) pixels of 128 B -- and the 9 taps read
  // shifted views of it, instead of 9 separate 256-row A tiles (9x the L2->LDS traffic)
  int halo_rows, halo_nbuf, n_cb;
  uint32_t halo_bytes;
  FastDiv div_hw2;  // halo pixel -> halo row (divide by WA + 2)
  FastDiv div_ha;   // global image row -> image (divide by HA)
  // EPI_STATS: non-null -> per-channel fp64 totals of y and y^2 (kernels.h BnFwdFuse) instead of `part`
  double* sacc;
  // K-concatenated second A operand (C64 loaders, one tap, dense 1x1 / stride 1 only): K-steps
  // past CA read a2[m][CA2] -- B rows are then [CA weights | CA2 weights] (kernels.h DgradFold)
  const uint16_t* a2;
  uint32_t a2_bytes;
  int CA2;
  const float* bias;  // optional per-output-channel fp32 bias added to the accumulators (EPI_BNB)
};

// epilogue variants of the NT kernel
constexpr int EPI_PLAIN = 0;  // store (+ optional addend)
constexpr int EPI_STATS = 1;  // + BN forward partial statistics (conv fwd)
constexpr int EPI_BNB = 2;    // + fused BN backward relu-mask and partial sums (conv dgrad)

#ifdef PDT_NT_TIMING
constexpr int kNtTimingSlots = 8 * 65536;
__device__ unsigned long long g_nt_timing[kNtTimingSlots];
#define NT_STAMP(i)                                                                      \
  do {                                                                                   \
    if (threadIdx.x == 0 && blockIdx.x < 65536) {                                        \
      g_nt_timing[blockIdx.x * 8 + (i)] = __builtin_amdgcn_s_memtime();                   \
      if ((i) == 0) {                                                                    \
        g_nt_timing[blockIdx.x * 8 + 6] = __builtin_amdgcn_s_memrealtime();               \
        g_nt_timing[blockIdx.x * 8 + 7] = (unsigned long long)__smid();                   \
      }                                                                                  \
    }                                                                                    \
  } while (0)
#else
#define NT_STAMP(i) do {} while (0)
#endif

int nt_timing_fetch(unsigned long long* host, int n) {
#ifdef PDT_NT_TIMING
  n = std::min(n, kNtTimingSlots);
  if (hipMemcpyFromSymbol(host, HIP_SYMBOL(g_nt_timing), (size_t)n * 8, 0, hipMemcpyDeviceToHost) != hipSuccess)
    return 0;
  return n;
#else
  (void)host; (void)n;
  return 0;
#endif
}


// LDS image of a [rows][64] bf16 tile: 128-B rows, 16-B chunk XOR-swizzled by (row>>1)&7.
// For the 16x16x32 fragment read (lane l: row l&15, chunk 4*ksub + (l>>4)) every ds_read_b128
// lane group then touches 16 distinct 16-B slots of the 256-B bank row: conflict-free.
__device__ __forceinline__ int swz128(int row, int chunk) {
  return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4);
}
// [rows][32] bf16 (K32 stages): 64-B rows, chunk XOR g(row>>2) with g = (0, 3, 2, 1).  A
// ds_read_b128 is serviced in four NON-contiguous 16-lane groups, {0-3,12-15,20-27},
// {4-11,16-19,28-31} and the same +32 (MI355X_MICROARCH §LDS): a fragment read's group holds rows
// {0-3,12-15} of one chunk and rows {4-11} of the next.  Slot = 4*(row&3) + (chunk ^ g): with
// g = (0,3,2,1) each of the four row classes maps {g0, g3, 1^g1, 1^g2} = {0,1,2,3}, so the
// group covers all 16 slots.  (The plain (row>>2)&3 XOR assumed contiguous groups and gave
// 2-way conflicts on every K32 fragment read: 3.9 vs 2.3 conflict cycles per LDS instruction
// against the K64 image on the layer1 1x1 forward, r2s3a.)
__device__ __forceinline__ int swz64_g(int row) { return (-(row >> 2)) & 3; }
__device__ __forceinline__ int swz64(int row, int chunk) {
  return row * 64 + ((chunk ^ swz64_g(row)) << 4);
}
// Epilogue staging image of a wave's (TM*16) x (TN*16) bf16 tile, rows of TN*32 bytes.  Writes
// are 8 B per lane (rows fr = lane & 15, one 16-B chunk per 32-lane half); reads are 16 B per lane
// over CH_PER_ROW consecutive chunks of consecutive rows, serviced in the non-contiguous lane
// groups {0-3,12-15,20-27} / {4-11,16-19,28-31} (+32).  XOR of the chunk index with row & 15
// (256-B rows) or (row >> 1) & 7 (128-B rows) puts both patterns on 16 distinct 16-B slots; the
// old +16 B row pad was conflict-free for the writes only.  PDT_EPI_SWZ=0 builds the padded image.
#ifndef PDT_EPI_SWZ
#define PDT_EPI_SWZ 1
#endif
template <int TN>
__device__ __forceinline__ int epi_off(int row, int chunk) {
  static_assert(TN == 4 || TN == 8, "epilogue staging image: 128- or 256-byte rows");
#if PDT_EPI_SWZ
  if constexpr (TN == 8) return row * 256 + ((chunk ^ (row & 15)) << 4);
  else return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4);
#else
  return row * (TN * 32 + 16) + (chunk << 4);
#endif
}

template <bool K32>
__device__ __forceinline__ int swz_row(int row, int chunk) {
  if constexpr (K32) return swz64(row, chunk);
  else return swz128(row, chunk);
}

// K32: a K-step is 32 bf16 (64-B operand rows) instead of 64 (128-B rows).  Same LDS per stage
// pair, so the ring can be twice as deep for the same footprint: a 4-stage K32 ring keeps three
// steps of loads in flight where the 2-stage K64 ring keeps one (one barrier per 32 of K).
template <int WM, int WN, int TM, int TN, int STAGES = 2, bool K32 = false>
struct NtCfg {
  static constexpr int NT = WM * WN * 64;
  static constexpr int WAVES = WM * WN;
  static constexpr int BM = WM * TM * 16;
  static constexpr int BN = WN * TN * 16;
  static constexpr int ROWB = K32 ? 64 : 128;  // bytes per operand row per K-step
  static constexpr int RPI = 1024 / ROWB;      // rows per LDS-DMA wave instruction (64 x 16 B)
  static constexpr int LPR = ROWB / 16;        // lanes per row in one instruction
  static constexpr int A_PW = BM / RPI / WAVES;  // instructions per wave per K-step
  static constexpr int B_PW = BN / RPI / WAVES;
  static_assert(A_PW * RPI * WAVES == BM && B_PW * RPI * WAVES == BN, "tile rows must split over waves");
  static constexpr int STAGE_BYTES = (BM + BN) * ROWB;
  static constexpr int PIPE_BYTES = STAGES * STAGE_BYTES;
  // bytes per epilogue staging row (pixel): unpadded with the XOR image (epi_off), else +16 B pad
  static constexpr int EPI_PITCH = TN * 16 * 2 + (PDT_EPI_SWZ ? 0 : 16);
  static constexpr int EPI_BYTES = WAVES * (TM * 16) * EPI_PITCH;
  static constexpr int SMEM = PIPE_BYTES > EPI_BYTES ? PIPE_BYTES : EPI_BYTES;
};


// Main loop: LDS-DMA staging (no VGPR round trip, no ds_write), the XOR swizzle applied on the
// SOURCE side (lane slot j of row r fetches chunk j ^ f(r)) so the lane-linear LDS image equals
// the swizzled image swz128() reads.  Two buffers: the DMA of tile k+1 is issued before the MFMAs
// of tile k; one vmcnt(0)+barrier per K-step.
// MFMA operands are swapped (A = weights, B = pixels) so each lane's 4 accumulator registers are
// 4 consecutive output channels of one pixel: the epilogue packs them into one 8-byte LDS write
// and the BN statistics reduce over the 16 pixel-lanes with DPP-friendly xor shuffles.
// Minimum waves per SIMD the register allocator must leave room for (launch bounds).  With the
// default (1) hipcc parks the accumulators in AGPRs and allocates 204-232 registers per lane for
// the 4-wave tiles (2 waves per SIMD); a floor of 2 gives the same code in 115 (stats / plain
// epilogue) and 168 (BN-backward epilogue) VGPRs, no spills, so the one-K-step 1x1 convs (whose
// LDS fits 4 blocks) run 3-4 blocks per CU: layer1 64->256 fwd 147 -> 130 us, 256->64 BN dgrad
// 234 -> 200 us, ResNet-50 step 20.50 -> 20.35 ms (r2v).  The 8-wave tile is LDS-bound at one
// block per CU either way.  PDT_NT_OCC4 / PDT_NT_OCC8 are build-time tuning knobs.
#ifndef PDT_NT_OCC4
#define PDT_NT_OCC4 2
#endif
#ifndef PDT_NT_OCC8
#define PDT_NT_OCC8 1
#endif
template <int WAVES, bool HALO>
constexpr int nt_min_waves() {
  return WAVES == 4 ? (HALO ? 2 : PDT_NT_OCC4) : PDT_NT_OCC8;
}

// NT epilogue (a device function so other NT-shaped kernels can share it): BN
// statistics (EPI_STATS) or the fused BN-backward mask / partial sums (EPI_BNB), bf16 staging
// through LDS (`smem`, idle pipeline buffers: every wave must be past its last fragment read)
// and 16-byte row stores.  Every thread of the workgroup calls it (it has block barriers).
// EPI_STATS: the BN statistics are summed in the store loop, from the bf16 chunks each lane
// stores -- the lane's 8 channels are fixed, so a chunk costs 8 unpacks + 4 v_pk_add_f32 + 4
// v_pk_fma_f32, and one shuffle reduction over the lanes sharing the channels follows (summing the
// fp32 accumulators before staging instead cost ~600 VALU + hazard nops per wave on the 256x256
// tile, as long as the main loop of a short-K 1x1 conv).  The bf16 statistics are those of the
// tensor the BN apply reads (torch's autocast semantics).


// BN statistics as fp64 totals (NtArgs::sacc), called by every thread of a workgroup after
// red[WM][2][BN] holds the workgroup's per-channel (sum, sum of squares) by wave row: one
// fire-and-forget agent-scope fp64 atomic add per channel and moment.  A one-block-per-256-channel
// launch (launch_bn_finalize_sums) turns the totals into the statistics and re-zeroes them --
// instead of bn_finalize's reduction over one partial per row tile (3136-6272 of them on layer 1).
// Precision: the totals are fp64, but each workgroup's contribution is an fp32 sum over its <= 256
// rows, so var = E[y^2] - mean^2 carries a relative error of roughly (mean / std)^2 * 2^-24 per
// tile sum (averaging down over the tiles) -- not fp64's 1e-16.  Pinned at |mean| / std up to ~100
// by tests/test_tiles_gpu.py::test_fwd_bn_fused_stats_far_from_zero_mean (invstd within 1e-3 of
// an fp64 two-pass reference over the same bf16 y).
template <class CFG, int WM>
__device__ __forceinline__ void nt_stats_atomic(const NtArgs& P, const float* red, int n0) {
  constexpr int BN = CFG::BN;
  const int t = threadIdx.x;
  const int col = n0 + t;
  if (t < BN && col < P.Nout) {
    float S = 0.f, Q = 0.f;
#pragma unroll
    for (int w = 0; w < WM; ++w) {
      S += red[(w * 2 + 0) * BN + t];
      Q += red[(w * 2 + 1) * BN + t];
    }
    // one [2][Nout] slot per XCD (workgroups are dealt to the 8 XCDs round-robin): 8x fewer adds
    // to each address than one shared total
    double* slot = P.sacc + (size_t)(blockIdx.x & 7) * 2 * P.Nout;
    __hip_atomic_fetch_add(slot + col, (double)S, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(slot + P.Nout + col, (double)Q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

template <class CFG, int WM, int WN, int TM, int TN, int EPI, int OP>
__device__ __forceinline__ void nt_epilogue(const NtArgs& P, v4f (&acc)[TM][TN], char* smem, int m0, int n0,
                                            int tmi) {
  constexpr int BM = CFG::BM, BN = CFG::BN;
  (void)BM;
  const int t = threadIdx.x;
  const int lane = t & 63, wid = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = wid % WM, wn = wid / WM;
  const int fr = lane & 15, fq = lane >> 4;
  // lane (fq, fr), register e of acc[i][j]: pixel i*16 + fr, channel j*16 + fq*4 + e
  const int wrow0 = m0 + wm * TM * 16;  // first GEMM row (pixel) of this wave
  const int wcol0 = n0 + wn * TN * 16;  // first output channel of this wave

  if constexpr (EPI == EPI_BNB) {
    if (P.bias != nullptr) {  // folded BN-backward constant term (DgradFold)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int col = wcol0 + j * 16 + fq * 4;
        const float4 bv = col < P.Nout ? *reinterpret_cast<const float4*>(P.bias + col)
                                       : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          if (wrow0 + i * 16 + fr < P.M) {  // rows past the GEMM stay 0 (the BN sums count them)
            acc[i][j][0] += bv.x; acc[i][j][1] += bv.y; acc[i][j][2] += bv.z; acc[i][j][3] += bv.w;
          }
        }
      }
    }
  }
  if constexpr (OP != OP_BF16) {
    // fp8: back to real units with the per-column factor (weight scale x activation scale)
    const float as = P.ascale != nullptr ? P.ascale[0] : 1.f;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col = wcol0 + j * 16 + fq * 4;
      float4 sc = col < P.Nout ? *reinterpret_cast<const float4*>(P.oscale + col)
                               : make_float4(0.f, 0.f, 0.f, 0.f);
      sc.x *= as; sc.y *= as; sc.z *= as; sc.w *= as;
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        acc[i][j][0] *= sc.x; acc[i][j][1] *= sc.y; acc[i][j][2] *= sc.z; acc[i][j][3] *= sc.w;
      }
    }
  }

  NT_STAMP(3);
  // stage the wave's pixels x channels tile as bf16 (8-byte writes), then 16-byte row stores
  char* ep = smem + wid * (TM * 16) * CFG::EPI_PITCH;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      uint2 v;
      v.x = pack2bf(acc[i][j][0], acc[i][j][1]);
      v.y = pack2bf(acc[i][j][2], acc[i][j][3]);
      *reinterpret_cast<uint2*>(ep + epi_off<TN>(i * 16 + fr, j * 2 + (fq >> 1)) + (fq & 1) * 8) = v;
    }
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): region is wave-private, no barrier needed
  __builtin_amdgcn_wave_barrier();
  constexpr int CH_PER_ROW = TN * 2;  // 16-B chunks per wave-tile row
  constexpr int CHUNKS = TM * 16 * CH_PER_ROW;
  static_assert(64 % CH_PER_ROW == 0, "a lane keeps one channel chunk across the store loop");
  // EPI_BNB: this lane's 8 channels are fixed (c = lane % CH_PER_ROW); per-lane partial sums
  float bmu[8], bsc[8], bsh[8], bsg[8], bsq[8];
  float bmu2[8], bsq2[8];   // EPI_BNB with bn_y2: the second BN's mean and sum g*y2
  const bool has_y2 = EPI == EPI_BNB && P.bn_y2 != nullptr;
  pdt_f2 st_s[4], st_q[4];  // EPI_STATS (store-loop form): the lane's 8 channels, as pairs
#pragma unroll
  for (int h = 0; h < 4; ++h) { st_s[h] = pdt_f2{0.f, 0.f}; st_q[h] = pdt_f2{0.f, 0.f}; }
  if constexpr (EPI == EPI_BNB) {
    const int colb = min(wcol0 + (lane % CH_PER_ROW) * 8, P.Nout - 8);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      bmu[q] = P.bn_stats[colb + q];
      bsc[q] = P.bn_stats[2 * P.Nout + colb + q];
      bsh[q] = P.bn_stats[3 * P.Nout + colb + q];
      bsg[q] = 0.f;
      bsq[q] = 0.f;
      bsq2[q] = 0.f;
      bmu2[q] = has_y2 ? P.bn_stats2[colb + q] : 0.f;
    }
  }
  // Two phases per batch of up to 8 chunks: first issue every global read the epilogue needs
  // (BN y / z, residual-gradient addend) -- bounds-checked buffer loads, OOB lanes read 0 --
  // then combine and store.  One exposed memory latency per batch instead of one per chunk (the
  // compiler cannot hoist a load above a store that may alias it); batches bound the registers.
  constexpr int IT_ALL = CHUNKS / 64;
#ifndef PDT_EPI_IT
#define PDT_EPI_IT 8
#endif
  constexpr int IT_MAX = PDT_EPI_IT;  // (y, z, addend) chunks in flight per lane and batch
  constexpr int IT = IT_ALL < IT_MAX ? IT_ALL : IT_MAX;
  static_assert(IT_ALL % IT == 0, "chunk batches");
  // The BN mask mode, the addend and the output addressing are wave-uniform: dispatch ONCE to a
  // copy of the batch loop specialised on them (per-element tests of kernel arguments cost ~6x
  // the SALU and 2.5x the VALU instructions of the plain epilogue, measured).
  //   DN: dense output (GEMM row == NHWC pixel) and, if any, an addend at the same offsets -- a
  //       chunk's offset is then the lane's base + a compile-time multiple of the row pitch (one
  //       add and one compare per chunk instead of the pixel decomposition's ~12 VALU).
  // Mask mode 3 (bitmask) masks the PACKED bf16 chunk: per pair of channels two sign-extended
  // bit fields merged by one v_bfi_b32 give the 32-bit keep-mask, so g is never unpacked, masked
  // and re-packed (the chunk was rounded to bf16 already: same bits as masking in fp32).
  auto run_batches = [&](auto mm_c, auto ha_c, auto dn_c, auto y2_c) {
    constexpr int MM = decltype(mm_c)::value;   // 0 none, 1 z > 0, 2 y*sc+sh > 0, 3 bitmask
    constexpr bool HA = decltype(ha_c)::value;  // residual-gradient addend
    constexpr bool DN = decltype(dn_c)::value;  // dense addressing fast path
    constexpr bool Y2 = decltype(y2_c)::value;  // second BN's y (bn_y2)
    constexpr int RSTEP = 64 / CH_PER_ROW;      // staging rows advanced per chunk slot
    const int c_l = lane % CH_PER_ROW, r_l = lane / CH_PER_ROW;
    const int col_l = wcol0 + c_l * 8;
    const int mrem = (col_l < P.Nout) ? P.M - (wrow0 + r_l) : 0;  // rows this lane may still touch
    const uint32_t off_l = ((uint32_t)(wrow0 + r_l) * (uint32_t)P.Nout + (uint32_t)col_l) * 2u;
    const uint32_t pitch = (uint32_t)P.Nout * 2u * RSTEP;  // bytes between a lane's chunks
#pragma unroll 1
    for (int b0 = 0; b0 < IT_ALL; b0 += IT) {
      uint32_t ooff[IT];  // byte offset of the chunk in the NHWC output (and y / z / addend), or OOB
      uint32_t aoff[IT];  // byte offset of the chunk in a compact (stride-2) addend, or OOB
      if constexpr (DN) {
        const uint32_t ob = off_l + (uint32_t)b0 * pitch;
#pragma unroll
        for (int it = 0; it < IT; ++it) {
          ooff[it] = (b0 + it) * RSTEP < mrem ? ob + (uint32_t)it * pitch : OOB;
          aoff[it] = ooff[it];
        }
      } else {
#pragma unroll
        for (int it = 0; it < IT; ++it) {
          const int qd = lane + (b0 + it) * 64;
          const int r = qd / CH_PER_ROW, c = qd - r * CH_PER_ROW;
          const int m = wrow0 + r;
          const int col = wcol0 + c * 8;
          ooff[it] = OOB;
          aoff[it] = OOB;
          if (m < P.M && col < P.Nout) {
            // 32-bit offsets: every operand is addressed through a buffer resource (< 4 GiB)
            uint32_t orow = (uint32_t)m;  // dense output (fwd, stride-1 dgrad): GEMM row == NHWC pixel
            if (!P.dense || (HA && P.add_sub)) {
              uint32_t n = fdiv((uint32_t)m, P.div_ij);
              uint32_t rem = (uint32_t)m - n * (uint32_t)P.Mij;
              uint32_t ii = fdiv(rem, P.div_j);
              uint32_t jj = rem - ii * (uint32_t)P.Mj;
              if (!P.dense)    // parity-class dgrad: scatter to (n, i*s + ph, j*s + pw)
                orow = (n * (uint32_t)P.OH + ii * (uint32_t)P.osh + (uint32_t)P.oph) * (uint32_t)P.OW +
                       jj * (uint32_t)P.osw + (uint32_t)P.opw;
              if (HA && P.add_sub) {
                // compact addend: (n, h/2, w/2) for even h and w.  Parity class (0, 0) of a stride-2
                // dgrad IS that grid (row m -> compact pixel m); other classes get nothing
                const int hh = P.dense ? (int)ii : (int)ii * P.osh + P.oph;
                const int ww = P.dense ? (int)jj : (int)jj * P.osw + P.opw;
                if (((hh | ww) & 1) == 0)
                  aoff[it] = (((n * (uint32_t)P.add_h + (uint32_t)(hh >> 1)) * (uint32_t)P.add_w + (uint32_t)(ww >> 1)) *
                                  (uint32_t)P.Nout + (uint32_t)col) * 2u;
              }
            }
            ooff[it] = (orow * (uint32_t)P.Nout + (uint32_t)col) * 2u;
            if (HA && !P.add_sub) aoff[it] = ooff[it];
          }
        }
      }
      v4i av[IT], yv[IT], zv[IT], y2v[Y2 ? IT : 1];
      if constexpr (HA) {
        const __amdgpu_buffer_rsrc_t rr = make_rsrc(P.addend, P.add_bytes);
#pragma unroll
        for (int it = 0; it < IT; ++it) av[it] = buf_load16(rr, aoff[it]);
      }
      if constexpr (EPI == EPI_BNB) {
        const __amdgpu_buffer_rsrc_t rr = make_rsrc(P.bn_y, P.o_bytes);
#pragma unroll
        for (int it = 0; it < IT; ++it) yv[it] = buf_load16(rr, ooff[it]);
        if constexpr (Y2) {
          const __amdgpu_buffer_rsrc_t r2 = make_rsrc(P.bn_y2, P.o_bytes);
#pragma unroll
          for (int it = 0; it < IT; ++it) y2v[it] = buf_load16(r2, ooff[it]);
        }
        if constexpr (MM == 1) {
          const __amdgpu_buffer_rsrc_t rz = make_rsrc(P.bn_z, P.o_bytes);
#pragma unroll
          for (int it = 0; it < IT; ++it) zv[it] = buf_load16(rz, ooff[it]);
        } else if constexpr (MM == 3) {  // 1 byte per 16-B chunk instead of the 16-B z chunk
          const __amdgpu_buffer_rsrc_t rz = make_rsrc(P.bn_z, P.o_bytes >> 4);
#pragma unroll
          for (int it = 0; it < IT; ++it)
            zv[it][0] = (int)__builtin_amdgcn_raw_buffer_load_b8(rz, ooff[it] == OOB ? OOB : ooff[it] >> 4, 0, 0);
        }
      }
#pragma unroll
      for (int it = 0; it < IT; ++it) {
        const int qd = lane + (b0 + it) * 64;
        const int r = qd / CH_PER_ROW, c = qd - r * CH_PER_ROW;
        v4i v = *reinterpret_cast<const v4i*>(ep + epi_off<TN>(r, c));
        if constexpr (HA) {  // fused residual-gradient sum (block input of a residual block)
          f8 a = unpack8(__builtin_bit_cast(uint4, v));
          const f8 b = unpack8(__builtin_bit_cast(uint4, av[it]));
#pragma unroll
          for (int q = 0; q < 8; ++q) a.v[q] += b.v[q];
          v = __builtin_bit_cast(v4i, pack8(a));
        }
        if constexpr (EPI == EPI_BNB) {
          // g = dx * relu'(unit output); g is bf16-exact (dx or 0), so the stored tensor and the
          // partial sums agree bit for bit with what the apply pass reads back.  OOB chunks read
          // y = 0 and contribute g = 0 (their accumulators are 0: rows/cols past the GEMM edge).
          if constexpr (MM == 3) {
            const int zb = zv[it][0];
#pragma unroll
            for (int h = 0; h < 4; ++h) {
              const uint32_t lo = (uint32_t)__builtin_amdgcn_sbfe(zb, 2 * h, 1);      // 0 or ~0
              const uint32_t hi = (uint32_t)__builtin_amdgcn_sbfe(zb, 2 * h + 1, 1);
              const uint32_t keep = (0x0000ffffu & lo) | (~0x0000ffffu & hi);         // v_bfi_b32
              v[h] = (int)((uint32_t)v[h] & keep);
            }
          }
          f8 a = unpack8(__builtin_bit_cast(uint4, v));
          const f8 yy = unpack8(__builtin_bit_cast(uint4, yv[it]));
          if constexpr (MM == 1 || MM == 2) {
            f8 zz;
            if constexpr (MM == 1) zz = unpack8(__builtin_bit_cast(uint4, zv[it]));
#pragma unroll
            for (int q = 0; q < 8; ++q) {
              bool on;
              if constexpr (MM == 1) on = zz.v[q] > 0.f;
              else on = fmaf(yy.v[q], bsc[q], bsh[q]) > 0.f;
              a.v[q] = on ? a.v[q] : 0.f;  // OOB: a == 0 and y == 0 -> contributes 0
            }
            v = __builtin_bit_cast(v4i, pack8(a));
          }
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            bsg[q] += a.v[q];
            bsq[q] = fmaf(a.v[q], yy.v[q], bsq[q]);  // sum g*y; the mean term comes off once below
          }
          if constexpr (Y2) {
            const f8 y2 = unpack8(__builtin_bit_cast(uint4, y2v[it]));
#pragma unroll
            for (int q = 0; q < 8; ++q) bsq2[q] = fmaf(a.v[q], y2.v[q], bsq2[q]);
          }
        }
        if constexpr (EPI == EPI_STATS) {
          // rows past the GEMM edge were staged as 0 (their accumulators are 0): no mask needed
#pragma unroll
          for (int h = 0; h < 4; ++h) {
            const uint32_t w = (uint32_t)v[h];
            const pdt_f2 a2 = {__uint_as_float(w << 16), __uint_as_float(w & 0xffff0000u)};
            st_s[h] += a2;
            st_q[h] = __builtin_elementwise_fma(a2, a2, st_q[h]);
          }
        }
        if (ooff[it] != OOB) *reinterpret_cast<v4i*>(reinterpret_cast<char*>(P.out) + ooff[it]) = v;
      }
    }
  };
  using M0 = std::integral_constant<int, 0>;
  using M1 = std::integral_constant<int, 1>;
  using M2 = std::integral_constant<int, 2>;
  using M3 = std::integral_constant<int, 3>;
  using HT = std::integral_constant<bool, true>;
  using HF = std::integral_constant<bool, false>;
  const bool has_add = P.addend != nullptr;
  const bool dense = P.dense && !(has_add && P.add_sub);
  auto with_dn = [&](auto mm, auto ha) {
    if (dense) run_batches(mm, ha, HT{}, HF{});
    else run_batches(mm, ha, HF{}, HF{});
  };
  if constexpr (EPI == EPI_BNB) {
    switch (P.bn_mask) {
      case 1: if (has_add) with_dn(M1{}, HT{}); else with_dn(M1{}, HF{}); break;
      case 2: if (has_add) with_dn(M2{}, HT{}); else with_dn(M2{}, HF{}); break;
      case 3:
        if (has_add && has_y2) {  // the hand-off dgrad of a downsampling block's output
          if (dense) run_batches(M3{}, HT{}, HT{}, HT{});
          else run_batches(M3{}, HT{}, HF{}, HT{});
        } else if (has_add) {
          with_dn(M3{}, HT{});
        } else {
          with_dn(M3{}, HF{});
        }
        break;
      default: if (has_add) with_dn(M0{}, HT{}); else with_dn(M0{}, HF{}); break;
    }
  } else {
    if (has_add) with_dn(M0{}, HT{}); else with_dn(M0{}, HF{});
  }
  if constexpr (EPI == EPI_STATS) {
    float s8[8], q8[8];
#pragma unroll
    for (int h = 0; h < 4; ++h) { s8[2 * h] = st_s[h].x; s8[2 * h + 1] = st_s[h].y; q8[2 * h] = st_q[h].x; q8[2 * h + 1] = st_q[h].y; }
    // lanes holding the same channel chunk (lane, lane + CH_PER_ROW, ...) -> the wave's TM*16 rows
#pragma unroll
    for (int o = CH_PER_ROW; o < 64; o <<= 1)
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        s8[q] += __shfl_xor(s8[q], o, 64);
        q8[q] += __shfl_xor(q8[q], o, 64);
      }
    const bool fused = P.sacc != nullptr;
    // partials path: M2 about the wave's mean (cancellation benign at <= 64 rows), then the WM wave
    // rows of the workgroup merge in LDS (Chan) into ONE partial per (row tile, channel), as
    // bn_finalize reads.  Fused path: plain sums and sums of squares, added to fp64 totals.
    const int valid = min(TM * 16, P.M - wrow0);  // <= 0: wave past the GEMM edge, contributes 0
    const float inv_valid = valid > 0 ? 1.f / (float)valid : 0.f;
    __syncthreads();  // every wave has finished reading its staging rows (red[] aliases them)
    float* red = reinterpret_cast<float*>(smem);  // [WM][2][BN]
    if (lane < CH_PER_ROW) {
      float m2[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) m2[q] = fused ? q8[q] : fmaxf(q8[q] - s8[q] * s8[q] * inv_valid, 0.f);
      float* rp = red + (wm * 2) * BN + wn * TN * 16 + lane * 8;
      *reinterpret_cast<float4*>(rp) = make_float4(s8[0], s8[1], s8[2], s8[3]);
      *reinterpret_cast<float4*>(rp + 4) = make_float4(s8[4], s8[5], s8[6], s8[7]);
      *reinterpret_cast<float4*>(rp + BN) = make_float4(m2[0], m2[1], m2[2], m2[3]);
      *reinterpret_cast<float4*>(rp + BN + 4) = make_float4(m2[4], m2[5], m2[6], m2[7]);
    }
    __syncthreads();
    if (fused) {
      nt_stats_atomic<CFG, WM>(P, red, n0);
    } else if (t < BN) {  // thread t merges channel n0 + t over the WM wave rows (fixed order)
      float sw[WM], qw[WM], nw[WM];
      float S = 0.f, Nr = 0.f;
#pragma unroll
      for (int w = 0; w < WM; ++w) {
        nw[w] = (float)max(0, min(TM * 16, P.M - (m0 + w * TM * 16)));
        sw[w] = red[(w * 2 + 0) * BN + t];
        qw[w] = red[(w * 2 + 1) * BN + t];
        S += sw[w];
        Nr += nw[w];
      }
      const float mean = S / Nr;  // Nr > 0: the tile's first wave row is inside the GEMM
      float Q = 0.f;
#pragma unroll
      for (int w = 0; w < WM; ++w) {
        if (nw[w] > 0.f) {
          const float d = sw[w] / nw[w] - mean;
          Q += qw[w] + nw[w] * d * d;
        }
      }
      const int col = n0 + t;
      if (col < P.Nout) {
        P.part[((int64_t)tmi * 2 + 0) * P.Nout + col] = S;
        P.part[((int64_t)tmi * 2 + 1) * P.Nout + col] = Q;
      }
    }
  }
  if constexpr (EPI == EPI_BNB) {
    // sum g*(y - mean) = sum g*y - mean * sum g per lane: one VALU per element less in the batch
    // loop above (the epilogue, not the MFMAs, bounds the short-K dgrads' issue)
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      bsq[q] = fmaf(-bmu[q], bsg[q], bsq[q]);
      bsq2[q] = fmaf(-bmu2[q], bsg[q], bsq2[q]);
    }
    // combine the lanes holding the same channel chunk (lane, lane+CH_PER_ROW, ...), then the
    // first CH_PER_ROW lanes write this wave's (rows group, channels) partials
#pragma unroll
    for (int o = CH_PER_ROW; o < 64; o <<= 1)
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        bsg[q] += __shfl_xor(bsg[q], o, 64);
        bsq[q] += __shfl_xor(bsq[q], o, 64);
      }
    if (has_y2)
#pragma unroll
      for (int o = CH_PER_ROW; o < 64; o <<= 1)
#pragma unroll
        for (int q = 0; q < 8; ++q) bsq2[q] += __shfl_xor(bsq2[q], o, 64);
    // then the WM wave rows of the workgroup are summed in LDS (fixed order): one partial per
    // (workgroup row tile, channel).  Waves past the GEMM edge hold zeros.
    __syncthreads();  // every wave has finished reading its staging rows (red[] aliases them)
    float* red = reinterpret_cast<float*>(smem);  // [WM][3][BN]
    if (lane < CH_PER_ROW) {
      float* rp = red + (wm * 3) * BN + wn * TN * 16 + lane * 8;
      *reinterpret_cast<float4*>(rp) = make_float4(bsg[0], bsg[1], bsg[2], bsg[3]);
      *reinterpret_cast<float4*>(rp + 4) = make_float4(bsg[4], bsg[5], bsg[6], bsg[7]);
      *reinterpret_cast<float4*>(rp + BN) = make_float4(bsq[0], bsq[1], bsq[2], bsq[3]);
      *reinterpret_cast<float4*>(rp + BN + 4) = make_float4(bsq[4], bsq[5], bsq[6], bsq[7]);
      if (has_y2) {
        *reinterpret_cast<float4*>(rp + 2 * BN) = make_float4(bsq2[0], bsq2[1], bsq2[2], bsq2[3]);
        *reinterpret_cast<float4*>(rp + 2 * BN + 4) = make_float4(bsq2[4], bsq2[5], bsq2[6], bsq2[7]);
      }
    }
    __syncthreads();
    if (t < BN && n0 + t < P.Nout) {
      float S = 0.f, Q = 0.f, Q2 = 0.f;
#pragma unroll
      for (int w = 0; w < WM; ++w) {
        S += red[(w * 3) * BN + t];
        Q += red[(w * 3 + 1) * BN + t];
        if (has_y2) Q2 += red[(w * 3 + 2) * BN + t];
      }
      if (has_y2) {  // the second BN's accumulator: same sum g, its own centred sum
        unsafeAtomicAdd(P.bn_acc2 + n0 + t, S);
        unsafeAtomicAdd(P.bn_acc2 + P.Nout + n0 + t, Q2);
      }
      if (P.bn_acc != nullptr) {  // the BN-backward apply reads the finished sums: no reduce launch
        unsafeAtomicAdd(P.bn_acc + n0 + t, S);
        unsafeAtomicAdd(P.bn_acc + P.Nout + n0 + t, Q);
      } else {
        float* pp = P.bn_part + ((int64_t)(P.bn_group0 + tmi) * 2) * P.Nout + n0 + t;
        pp[0] = S;
        pp[P.Nout] = Q;
      }
    }
  }
}

template <int WM, int WN, int TM, int TN, int STAGES, bool C64, int EPI, int OP = OP_BF16, bool HALO = false,
          bool K32 = false>
__global__ void __launch_bounds__(WM * WN * 64, (nt_min_waves<WM * WN, HALO>())) igemm_nt_kernel(const NtArgs P) {
  static_assert(!HALO || (C64 && OP == OP_BF16), "halo staging: bf16, 64-channel blocks");
  static_assert(!K32 || (OP == OP_BF16 && !HALO), "K32 stages: bf16 per-tap staging only");
  using CFG = NtCfg<WM, WN, TM, TN, STAGES, K32>;
  constexpr int BM = CFG::BM, BN = CFG::BN, A_PW = CFG::A_PW, B_PW = CFG::B_PW;
  constexpr int RPI = CFG::RPI, LPR = CFG::LPR;
  constexpr int EB = OP == OP_BF16 ? 2 : 1;  // bytes per element
  constexpr int KE = CFG::ROWB / EB;         // elements per K-step (one operand row)
  constexpr int CE = 16 / EB;                // elements per 16-byte chunk
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int ntn = (P.Nout + BN - 1) / BN;
  const int ntm = (P.M + BM - 1) / BM;
  const int bid = xcd_remap(blockIdx.x, ntm * ntn);
  const int tmi = bid / ntn, tni = bid - (bid / ntn) * ntn;
  const int m0 = tmi * BM, n0 = tni * BN;

  NT_STAMP(0);
  const int t = threadIdx.x;
  // wave id through readfirstlane: uniform for the compiler, so every LDS-DMA destination
  // (tile base + wave slot) is scalar math + one m0 write, no VGPR add + readfirstlane per load
  const int lane = t & 63, wid = __builtin_amdgcn_readfirstlane(t >> 6);
  const int lr = lane / LPR, lj = lane % LPR;  // row within a DMA instruction, LDS chunk slot
  // source chunk that lands in LDS slot lj of row `row` (the read side applies the same XOR)
  auto src_chunk = [&](int row) { return K32 ? (lj ^ swz64_g(row)) : (lj ^ ((row >> 1) & 7)); };

  const __amdgpu_buffer_rsrc_t ra = make_rsrc(P.a, P.a_bytes);
  const __amdgpu_buffer_rsrc_t rb = make_rsrc(P.b, P.b_bytes);
  const __amdgpu_buffer_rsrc_t ra2 = make_rsrc(P.a2, P.a2_bytes);

  // A rows (pixels) and B rows (output channels) this lane fetches, fixed over the K loop
  // a_base: byte offset of (h0, w0, this lane's chunk) -- a tap adds the uniform scalar
  // ((dr*WA + ds)*CA + chb)*2; only the bounds test on (h0+dr, w0+ds) stays per lane.
  int a_pix[A_PW], a_h0[A_PW], a_w0[A_PW], a_c[A_PW], a_base[A_PW];
#pragma unroll
  for (int i = 0; i < A_PW; ++i) {
    const int row = (wid * A_PW + i) * RPI + lr;
    a_c[i] = src_chunk(row);
    const int m = m0 + row;
    if (m < P.M) {
      uint32_t n = fdiv((uint32_t)m, P.div_ij);
      uint32_t rem = (uint32_t)m - n * (uint32_t)P.Mij;
      uint32_t ii = fdiv(rem, P.div_j);
      uint32_t jj = rem - ii * (uint32_t)P.Mj;
      a_pix[i] = (int)n * P.HA * P.WA;
      a_h0[i] = (int)ii * P.ash + P.aoff_h;
      a_w0[i] = (int)jj * P.asw + P.aoff_w;
    } else {
      a_pix[i] = 0; a_h0[i] = -(1 << 20); a_w0[i] = 0;
    }
    a_base[i] = (a_pix[i] + a_h0[i] * P.WA + a_w0[i]) * P.CA * EB + a_c[i] * 16;
  }
  // second A operand: GEMM row m == pixel m (dense 1x1); rows >= M lie past a2_bytes and read 0
  int a2_base[A_PW];
#pragma unroll
  for (int i = 0; i < A_PW; ++i) a2_base[i] = (m0 + (wid * A_PW + i) * RPI + lr) * P.CA2 * EB + a_c[i] * 16;
  int b_row[B_PW], b_c[B_PW];
#pragma unroll
  for (int i = 0; i < B_PW; ++i) {
    const int row = (wid * B_PW + i) * RPI + lr;
    b_c[i] = src_chunk(row);
    const int n = n0 + row;
    b_row[i] = n < P.Nout ? n * P.Kg : -1;
  }

  const int nk = C64 ? P.ntaps * (P.CA / KE) + (P.a2 != nullptr ? P.CA2 / KE : 0) : (P.Kg + KE - 1) / KE;

  // C64 path: per A row, bit t of a_inv = tap t (= ti*tns + tj) reads outside the image.  Built
  // once from the separable row / column validity; a K-step then turns it into a 0 / all-ones
  // poison with one bit-field extract and ORs it into the offset (all-ones >= num_records: the
  // buffer load returns 0) -- 3 VALU per row instead of two adds, two compares and a select.
  // Closed form, branch-free: along one axis the valid taps t (base + step*t in [0, extent),
  // step = +-1) form one interval [lo, hi); its bit run is (1<<hi) - (1<<lo).  The 2-D mask is
  // the column run replicated at the valid tap rows: wm * sum_{ti valid} 2^(ti*tns).
  uint32_t a_inv[A_PW];
  if constexpr (C64) {
    const int nr = P.tnr, ns = P.tns;
    const uint32_t rep1 = 1u << ns, rep2 = 1u << (2 * ns);  // tap rows 1, 2 (tnr <= 3 fast path)
#pragma unroll
    for (int i = 0; i < A_PW; ++i) {
      const int hb = a_h0[i] + P.dr0, wb = a_w0[i] + P.ds0;
      const int hlo = P.dstep > 0 ? max(0, -hb) : max(0, hb - P.HA + 1);
      const int hhi = P.dstep > 0 ? min(nr, P.HA - hb) : min(nr, hb + 1);
      const int wlo = P.dstep > 0 ? max(0, -wb) : max(0, wb - P.WA + 1);
      const int whi = P.dstep > 0 ? min(ns, P.WA - wb) : min(ns, wb + 1);
      const uint32_t hm = hhi > hlo ? (1u << (hhi & 31)) - (1u << (hlo & 31)) : 0u;
      const uint32_t wm = whi > wlo ? (1u << (whi & 31)) - (1u << (wlo & 31)) : 0u;
      uint32_t spread;
      if (nr <= 3) {
        spread = (hm & 1u) | ((hm & 2u) ? rep1 : 0u) | ((hm & 4u) ? rep2 : 0u);
      } else {
        spread = 0u;
        for (int ti = 0; ti < nr; ++ti) spread |= ((hm >> ti) & 1u) << (ti * ns);
      }
      a_inv[i] = ~(wm * spread);
    }
  }
  // c8 loader (non-C64, 8-channel source): per row the first source row of its chunk's tap and
  // the byte offset of that tap (or OOB when the tap column falls outside the image)
  int a_c8h[A_PW], a_c8o[A_PW];
  if constexpr (!C64) {
    if (P.c8) {
#pragma unroll
      for (int i = 0; i < A_PW; ++i) {
        const int r0 = a_c[i] / P.S, s0 = a_c[i] - r0 * P.S;
        const int w = a_w0[i] + s0;
        a_c8h[i] = a_h0[i] + r0;
        a_c8o[i] = (unsigned)w < (unsigned)P.WA ? ((a_pix[i] + a_c8h[i] * P.WA + w) * 8 * EB) : (int)OOB;
      }
    }
  }
  // K-step -> (tap row ti, tap column tj, channel block chb) advanced incrementally (issue() is
  // called for consecutive K-steps): no scalar divisions in the loop
  int k_ti = 0, k_tj = 0, k_chb = 0;

  // One LDS-DMA wave instruction ("piece" q < A_PW + B_PW) of K-step kt into stage `buf`;
  // `valid` false turns it into an all-OOB load (writes zeros, touches no memory).  C64: the
  // tap / channel-block state (k_*) is that of step kt; advance() moves it on.  (Interleaving
  // the pieces with the MFMAs instead of issuing a step's pieces as one burst was measured at
  // -1% in-step, r2ac: profiles/r2_nt_mainloop_experiments.md.)
  auto piece = [&](int kt, int buf, int q, bool valid) {
    char* As = smem + buf * CFG::STAGE_BYTES;
    char* Bs = As + BM * CFG::ROWB;
    if constexpr (C64) {
      const int tap = k_ti * P.tns + k_tj;
      if (q < A_PW && k_chb >= P.CA) {  // K-concatenated second operand (P.a2)
        const int i = q;
        glds16(ra2, As + (wid * A_PW + i) * 1024, valid ? (uint32_t)(a2_base[i] + (k_chb - P.CA) * EB) : OOB);
      } else if (q < A_PW) {
        const int i = q;
        const int dr = P.dr0 + k_ti * P.dstep, ds = P.ds0 + k_tj * P.dstep;
        const int tdelta = ((dr * P.WA + ds) * P.CA + k_chb) * EB;
        const uint32_t poison = (uint32_t)__builtin_amdgcn_sbfe((int)a_inv[i], (unsigned)tap, 1u) |
                                (valid ? 0u : 0xffffffffu);
        const uint32_t off = (uint32_t)(a_base[i] + tdelta) | poison;
        glds16(ra, As + (wid * A_PW + i) * 1024, off);
      } else {
        const int i = q - A_PW;
        const int tbo = ((P.tr0 + k_ti * P.tstep) * P.S + (P.ts0 + k_tj * P.tstep)) * P.CA + k_chb;
        uint32_t off = (valid && b_row[i] >= 0) ? (uint32_t)((b_row[i] + tbo) * EB + b_c[i] * 16) : OOB;
        glds16(rb, Bs + (wid * B_PW + i) * 1024, off);
      }
    } else if (P.c8) {
      // 8-channel source (the stem's super-pixel image): each 16-B chunk of a K-step is one
      // whole tap, tap = kt*8 + chunk, and the filter width divides 8, so a K-step advances
      // the source row by 8/S filter rows: offset = lane constant + kt * row step
      if (q < A_PW) {
        const int i = q;
        const int h = a_c8h[i] + kt * P.c8_rows;
        const bool ok = (unsigned)h < (unsigned)P.HA && a_c[i] < P.ntaps - kt * 8;
        glds16(ra, As + (wid * A_PW + i) * 1024, ok ? (uint32_t)(a_c8o[i] + kt * P.c8_step) : OOB);
      } else {
        const int i = q - A_PW;
        const int kk = kt * KE + b_c[i] * CE;
        uint32_t off = (kk < P.Kg && b_row[i] >= 0) ? (uint32_t)((b_row[i] + kk) * EB) : OOB;
        glds16(rb, Bs + (wid * B_PW + i) * 1024, off);
      }
    } else {
      if (q < A_PW) {
        const int i = q;
        const int kk = kt * KE + a_c[i] * CE;
        const int tap = (int)fdiv((uint32_t)kk, P.div_ca);  // mul-hi, not a runtime divide
        const int ch = kk - tap * P.CA;
        const int r = (int)fdiv((uint32_t)tap, P.div_s);
        const int s = tap - r * P.S;
        // tap (r, s) reads A at (dr0 + r*dstep, ds0 + s*dstep): forward (0, +1) or a stride-1
        // dgrad (pad, -1)
        int h = a_h0[i] + P.dr0 + r * P.dstep, w = a_w0[i] + P.ds0 + s * P.dstep;
        bool ok = kk < P.Kg && (unsigned)h < (unsigned)P.HA && (unsigned)w < (unsigned)P.WA;
        uint32_t off = ok ? (uint32_t)(((a_pix[i] + h * P.WA + w) * P.CA + ch) * EB) : OOB;
        glds16(ra, As + (wid * A_PW + i) * 1024, off);
      } else {
        const int i = q - A_PW;
        const int kk = kt * KE + b_c[i] * CE;
        uint32_t off = (kk < P.Kg && b_row[i] >= 0) ? (uint32_t)((b_row[i] + kk) * EB) : OOB;
        glds16(rb, Bs + (wid * B_PW + i) * 1024, off);
      }
    }
  };
  auto advance = [&]() {
    if constexpr (C64) {
      k_chb += KE;
      if (k_chb == P.CA && P.a2 == nullptr) {  // with a2 (one tap) the channel index runs on past CA
        k_chb = 0;
        if (++k_tj == P.tns) { k_tj = 0; ++k_ti; }
      }
    }
  };
  auto issue = [&](int kt, int buf) {
#pragma unroll
    for (int q = 0; q < A_PW + B_PW; ++q) piece(kt, buf, q, true);
    advance();
  };

  const int wm = wid % WM, wn = wid / WM;
  const int fr = lane & 15, fq = lane >> 4;

  v4f acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = v4f{0.f, 0.f, 0.f, 0.f};

  if constexpr (HALO) {
    // ------------------------------------------------ halo main loop (3x3 / s1 / same size)
    // LDS: [halo buffers][B stage 0][B stage 1][zero row].  K-steps run channel block (outer) x
    // tap (inner); B moves one [BN][64] tile per step (2 buffers), the halo of the next channel
    // block is fetched while the current one's 9 taps compute (2 buffers) or after them (1).
    const int WP = P.WA + 2;                        // halo row pitch in pixels (zero pad columns)
    const int g_first = (int)fdiv((uint32_t)m0, P.div_j);  // first global image row (n*HA + h)
    const int NH = P.M / P.WA;                      // global rows of the activation
    char* hbase = smem;
    char* bbase = smem + P.halo_nbuf * P.halo_bytes;
    char* zrow = bbase + 2 * BN * 128;
    if (t < 8) *reinterpret_cast<v4i*>(zrow + t * 16) = v4i{0, 0, 0, 0};
    // this lane's fragment pixels: halo pixel of the centre tap + which vertical taps stay inside
    // its image (a halo row above / below can belong to the neighbouring image: read zeros)
    int hp0[TM];
    uint32_t vrow[TM];  // bit 0: row above inside the image, bit 1: row below, bit 2: pixel < M
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int p = m0 + wm * TM * 16 + i * 16 + fr;
      if (p < P.M) {
        const uint32_t g = fdiv((uint32_t)p, P.div_j);
        const int w = p - (int)g * P.WA;
        const int h = (int)(g - fdiv(g, P.div_ha) * (uint32_t)P.HA);
        hp0[i] = ((int)g - g_first + 1) * WP + w + 1;
        vrow[i] = 4u | (h > 0 ? 1u : 0u) | (h + 1 < P.HA ? 2u : 0u);
      } else {
        hp0[i] = WP + 1;
        vrow[i] = 0u;  // rows past the GEMM: every tap reads zeros
      }
    }
    const int hpix = P.halo_rows * WP;
    const int nq = (hpix + 7) / 8;  // 1-KiB DMA instructions per halo
    auto issue_halo = [&](int cb, int hb) {
      char* dst = hbase + hb * P.halo_bytes;
      for (int q = wid; q < nq; q += CFG::WAVES) {
        const int hp = q * 8 + lr;
        const int hr = (int)fdiv((uint32_t)hp, P.div_hw2);
        const int col = hp - hr * WP - 1;
        const int g = g_first - 1 + hr;
        const bool ok = hp < hpix && g >= 0 && g < NH && (unsigned)col < (unsigned)P.WA;
        const int ch = lj ^ ((hp >> 1) & 7);
        const uint32_t off = ok ? (uint32_t)((((int64_t)g * P.WA + col) * P.CA + cb * 64 + ch * 8) * 2) : OOB;
        glds16(ra, dst + q * 1024, off);
      }
    };
    auto issue_b = [&](int ti, int tj, int cb, int bb) {
      char* Bs = bbase + bb * BN * 128;
      const int tbo = ((P.tr0 + ti * P.tstep) * P.S + (P.ts0 + tj * P.tstep)) * P.CA + cb * 64;
#pragma unroll
      for (int i = 0; i < B_PW; ++i) {
        const uint32_t off = b_row[i] >= 0 ? (uint32_t)((b_row[i] + tbo) * 2 + b_c[i] * 16) : OOB;
        glds16(rb, Bs + (wid * B_PW + i) * 1024, off);
      }
    };
    const int ntap = P.tnr * P.tns;
    const int nk_h = ntap * P.n_cb;
    issue_halo(0, 0);
    issue_b(0, 0, 0, 0);
    wait_vm<0>();
    __syncthreads();  // zero row + first tiles visible
    int ti = 0, tj = 0, cb = 0;      // K-step kt = cb * ntap + ti * tns + tj
    int ni = 0, nj = 0, ncb = 0;     // the next step's (tap row, tap col, channel block)
    for (int kt = 0; kt < nk_h; ++kt) {
      // next step's coordinates
      ni = ti; nj = tj + 1; ncb = cb;
      if (nj == P.tns) { nj = 0; if (++ni == P.tnr) { ni = 0; ++ncb; } }
      const bool more = kt + 1 < nk_h;
      const bool new_cb = more && ncb != cb;
      if (more) {
        issue_b(ni, nj, ncb, (kt + 1) & 1);
        if (new_cb && P.halo_nbuf == 2) issue_halo(ncb, ncb & 1);
      }
      const int dr = P.aoff_h + P.dr0 + ti * P.dstep;  // -1, 0 or +1
      const int ds = P.aoff_w + P.ds0 + tj * P.dstep;
      const int dtap = dr * WP + ds;
      const uint32_t need = 4u | (dr < 0 ? 1u : (dr > 0 ? 2u : 0u));
      const char* Hs = hbase + (P.halo_nbuf == 2 ? (cb & 1) : 0) * P.halo_bytes;
      const char* Bs = bbase + (kt & 1) * BN * 128;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int kc = ks * 4 + fq;
        v4i af[TM], bfr[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const int hp = hp0[i] + dtap;
          const bool ok = (vrow[i] & need) == need;
          const char* src = ok ? Hs + hp * 128 + ((kc ^ ((hp >> 1) & 7)) << 4) : zrow + kc * 16;
          af[i] = *reinterpret_cast<const v4i*>(src);
        }
#pragma unroll
        for (int j = 0; j < TN; ++j)
          bfr[j] = *reinterpret_cast<const v4i*>(Bs + swz128(wn * TN * 16 + j * 16 + fr, kc));
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[i][j] = mfma16(bfr[j], af[i], acc[i][j]);
      }
      if (new_cb && P.halo_nbuf == 1) {  // single halo buffer: refill after every wave read it
        lds_barrier();
        issue_halo(ncb, 0);
      }
      wait_vm<0>();
      lds_barrier();
      ti = ni; tj = nj; cb = ncb;
    }
  } else {
  constexpr int LPS = A_PW + B_PW;
#pragma unroll
  for (int p = 0; p < STAGES - 1; ++p)
    if (p < nk) issue(p, p);
  wait_steps<LPS>(min(nk, STAGES - 1) - 1);
  lds_barrier();
  NT_STAMP(1);
  int cur = 0, nxt = STAGES - 1;
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + STAGES - 1 < nk) issue(kt + STAGES - 1, nxt);
    const char* As = smem + cur * CFG::STAGE_BYTES;
    const char* Bs = As + BM * CFG::ROWB;
    if constexpr (OP == OP_BF16) {
#pragma unroll
      for (int ks = 0; ks < KE / 32; ++ks) {
        const int kc = ks * 4 + fq;
        v4i af[TM], bfr[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
          af[i] = *reinterpret_cast<const v4i*>(As + swz_row<K32>(wm * TM * 16 + i * 16 + fr, kc));
#pragma unroll
        for (int j = 0; j < TN; ++j)
          bfr[j] = *reinterpret_cast<const v4i*>(Bs + swz_row<K32>(wn * TN * 16 + j * 16 + fr, kc));
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[i][j] = mfma16(bfr[j], af[i], acc[i][j]);
      }
    } else {
      // lane group fq owns bytes 32*fq .. +31 of the row = chunks 2fq, 2fq+1
      v8i af[TM], bfr[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int row = wm * TM * 16 + i * 16 + fr;
        const v4i lo = *reinterpret_cast<const v4i*>(As + swz128(row, 2 * fq));
        const v4i hi = *reinterpret_cast<const v4i*>(As + swz128(row, 2 * fq + 1));
        af[i] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int row = wn * TN * 16 + j * 16 + fr;
        const v4i lo = *reinterpret_cast<const v4i*>(Bs + swz128(row, 2 * fq));
        const v4i hi = *reinterpret_cast<const v4i*>(Bs + swz128(row, 2 * fq + 1));
        bfr[j] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = mfma_f8<OP>(bfr[j], af[i], acc[i][j]);
    }
    wait_steps<LPS>(min(nk - 1, kt + STAGES - 1) - (kt + 1));
    lds_barrier();
    cur = cur + 1 == STAGES ? 0 : cur + 1;
    nxt = nxt + 1 == STAGES ? 0 : nxt + 1;
  }
  }  // !HALO

  // --------------------------------------------------------------- epilogue
  NT_STAMP(2);
  nt_epilogue<CFG, WM, WN, TM, TN, EPI, OP>(P, acc, smem, m0, n0, tmi);
  NT_STAMP(4);
}


// ============================================================================
//          NT 256x256, quadrant-phased pipeline (long-K fwd / dgrad, bf16)
// ============================================================================
// The 2-stage NT main loop above issues step k+1 at the top of step k and drains every DMA
// (vmcnt 0) at its bottom: a load has exactly one K-step of MFMA time to land, and on the
// 1-block-per-CU 256x256 tile that step is ~1 us -- about one L2->LDS DMA latency under load, so
// long-K GEMMs stall once per step (4096^3: 642 TF/s vs hipBLASLt 1,524).
//
// This kernel splits each 64-deep K-step of the 256x256 (or 128x128) tile into FOUR phases, one per output
// quadrant (X half hx, W half hw), so a quarter tile (one half of one operand, 16 KB) is dead as
// soon as its last phase has read it, and is refilled right then with the same quarter of step
// s+2 (two LDS stages, 128 KB):
//     P0: Q(0,0)  reads X0, W0 (fragments kept in registers)  -> both dead
//     P1: Q(0,1)  reads W1 (kept), reuses X0                    -> issue X0(s+2), W0(s+2)
//     P2: Q(1,0)  reads X1 (kept), reuses W0                    -> issue W1(s+2)
//     P3: Q(1,1)  reuses X1, W1 (no LDS reads)                  -> issue X1(s+2)
// Every quarter is issued 7 phases (1.75 K-steps) before its first read, in the order the next
// steps consume them, and each phase waits with a COUNTED vmcnt for exactly the quarters it
// reads (12 / 10 / 12 glds younger than them), never vmcnt(0): loads stay in flight across the
// barriers.  One barrier per phase covers both hazards: RAW (every wave's DMA pieces of the
// quarters read in this phase have landed: each wave's counted wait precedes it) and WAR (every
// wave finished reading the quarter refilled in this phase: reads are consumed, lgkmcnt 0, by the
// previous phase's MFMAs).  Steps past the end issue all-OOB pieces (zero fill, no memory
// traffic) so the counts stay static.
// Rows are permuted so that each wave's 4 quadrant sub-tiles form ONE contiguous 128x64 output
// tile (8 waves = 2 (M) x 4 (N)): X half hx holds GEMM rows {wm*128 + hx*64 + [0,64)}, W half
// hw holds channels {wn*64 + hw*32 + [0,32)}, so nt_epilogue runs unchanged (WM 2, WN 4,

// Geometry: WM x WN waves, each owning a contiguous (2*TMQ*16) x (2*TNQ*16) output tile made of
// its four quadrant sub-tiles (TMQ x TNQ MFMA tiles each).  256x256: 8 waves (2 x 4), TMQ 4,
// TNQ 2 (one block per CU, 128 KB of LDS).  128x128: 4 waves (2 x 2), TMQ = TNQ = 2 (64 KB, two
// blocks per CU).  A quarter is always BM/2 (or BN/2) rows x 128 B = 2 DMA pieces per wave.
template <int WM, int WN, int TMQ, int TNQ>
struct NtqCfg {
  static constexpr int WAVES = WM * WN, NT = WAVES * 64;
  static constexpr int BM = WM * TMQ * 32, BN = WN * TNQ * 32;
  static constexpr int QX = BM / 2 * 128, QW = BN / 2 * 128;  // quarter bytes
  static constexpr int STAGE = 2 * QX + 2 * QW;
  static_assert(QX == WAVES * 2048 && QW == WAVES * 2048, "a quarter is two 1-KiB DMA pieces per wave");
  using Epi = NtCfg<WM, WN, 2 * TMQ, 2 * TNQ, 2, false>;
  static constexpr int SMEM = 2 * STAGE > Epi::EPI_BYTES ? 2 * STAGE : Epi::EPI_BYTES;
  static constexpr int MIN_WAVES = WAVES == 8 ? 1 : 2;  // waves per SIMD: 1 or 2 blocks per CU
};

// OP: bf16 (a 128-B K-step = 64 elements = two 16x16x32 MFMAs per tile pair) or fp8 (128
// elements = one MX-rate 16x16x128 MFMA, operand = 32 B per lane: chunks 2fq, 2fq+1)
template <int WM, int WN, int TMQ, int TNQ, int EPI, int OP = OP_BF16>
__global__ void __launch_bounds__(WM * WN * 64, (NtqCfg<WM, WN, TMQ, TNQ>::MIN_WAVES))
    igemm_ntq_kernel(const NtArgs P) {
  using Q = NtqCfg<WM, WN, TMQ, TNQ>;
  using CFG = typename Q::Epi;
  constexpr int BM = Q::BM, BN = Q::BN, QX = Q::QX, QW = Q::QW, STAGE = Q::STAGE;
  constexpr int HX = BM / WM / 2, HW = BN / WN / 2;  // rows of one wave's quadrant sub-tile
  static_assert(CFG::BM == BM && CFG::BN == BN, "ntq geometry");
  constexpr int EB = OP == OP_BF16 ? 2 : 1, KE = 128 / EB;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int ntn = (P.Nout + BN - 1) / BN;
  const int ntm = (P.M + BM - 1) / BM;
  const int bid = xcd_remap(blockIdx.x, ntm * ntn);
  const int tmi = bid / ntn, tni = bid - (bid / ntn) * ntn;
  const int m0 = tmi * BM, n0 = tni * BN;

  const int t = threadIdx.x;
  const int lane = t & 63, wid = __builtin_amdgcn_readfirstlane(t >> 6);
  const int lr = lane >> 3, lj = lane & 7;  // row within a DMA instruction (8 rows), LDS chunk slot
  const __amdgpu_buffer_rsrc_t ra = make_rsrc(P.a, P.a_bytes);
  const __amdgpu_buffer_rsrc_t rb = make_rsrc(P.b, P.b_bytes);
  const __amdgpu_buffer_rsrc_t ra2 = make_rsrc(P.a2, P.a2_bytes);

  // this lane's DMA rows: piece i (0, 1) of half h covers half-local rows r = (wid*2 + i)*8 + lr;
  // half-local row r of X half h is GEMM row (r / HX)*2*HX + h*HX + r % HX (wave-row blocks), of W
  // half h channel (r / HW)*2*HW + h*HW + r % HW
  int a_base[2][2], a2_base[2][2], b_row[2][2], b_c[2][2];
  uint32_t a_inv[2][2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r = (wid * 2 + i) * 8 + lr;
      const int sc = lj ^ ((r >> 1) & 7);  // source chunk landing in slot lj (read side: swz128)
      b_c[h][i] = sc;
      const int m = m0 + (r / HX) * 2 * HX + h * HX + (r % HX);
      int pix = 0, h0 = -(1 << 20), w0 = 0;
      if (m < P.M) {
        const uint32_t n = fdiv((uint32_t)m, P.div_ij);
        const uint32_t rem = (uint32_t)m - n * (uint32_t)P.Mij;
        const uint32_t ii = fdiv(rem, P.div_j);
        const uint32_t jj = rem - ii * (uint32_t)P.Mj;
        pix = (int)n * P.HA * P.WA;
        h0 = (int)ii * P.ash + P.aoff_h;
        w0 = (int)jj * P.asw + P.aoff_w;
      }
      a_base[h][i] = (pix + h0 * P.WA + w0) * P.CA * EB + sc * 16;
      a2_base[h][i] = m * P.CA2 * EB + sc * 16;  // dense 1x1: row m == pixel m; m >= M reads 0
      // tap validity bitmask (see igemm_nt_kernel): bit t set = tap t reads outside the image
      const int nr = P.tnr, ns = P.tns;
      const int hb = h0 + P.dr0, wb = w0 + P.ds0;
      const int hlo = P.dstep > 0 ? max(0, -hb) : max(0, hb - P.HA + 1);
      const int hhi = P.dstep > 0 ? min(nr, P.HA - hb) : min(nr, hb + 1);
      const int wlo = P.dstep > 0 ? max(0, -wb) : max(0, wb - P.WA + 1);
      const int whi = P.dstep > 0 ? min(ns, P.WA - wb) : min(ns, wb + 1);
      const uint32_t hm = hhi > hlo ? (1u << (hhi & 31)) - (1u << (hlo & 31)) : 0u;
      const uint32_t wmk = whi > wlo ? (1u << (whi & 31)) - (1u << (wlo & 31)) : 0u;
      uint32_t spread = 0u;
      for (int ti = 0; ti < nr; ++ti) spread |= ((hm >> ti) & 1u) << (ti * ns);
      a_inv[h][i] = ~(wmk * spread);
      const int ch = n0 + (r / HW) * 2 * HW + h * HW + (r % HW);
      b_row[h][i] = ch < P.Nout ? ch * P.Kg : -1;
    }

  // K-step state of the NEXT step to issue (ti, tj, channel block), advanced once per step
  const int nk = P.ntaps * (P.CA / KE) + (P.a2 != nullptr ? P.CA2 / KE : 0);
  int q_ti = 0, q_tj = 0, q_chb = 0, q_kt = 0;
  auto advance = [&]() {
    ++q_kt;
    q_chb += KE;
    if (q_chb == P.CA && P.a2 == nullptr) {  // with a2 (one tap) the channel index runs on past CA
      q_chb = 0;
      if (++q_tj == P.tns) { q_tj = 0; ++q_ti; }
    }
  };
  // quarter (operand X = 0 / W = 1, half h) of the step held by the tracker, into stage `st`
  auto issue = [&](int op, int h, int st) {
    const bool valid = q_kt < nk;
    char* dst = smem + st * STAGE + (op == 0 ? h * QX : 2 * QX + h * QW) + wid * 2048;
    if (op == 0 && q_chb >= P.CA) {  // K-concatenated second operand (P.a2)
#pragma unroll
      for (int i = 0; i < 2; ++i)
        glds16(ra2, dst + i * 1024, valid ? (uint32_t)(a2_base[h][i] + (q_chb - P.CA) * EB) : OOB);
    } else if (op == 0) {
      const int tap = q_ti * P.tns + q_tj;
      const int dr = P.dr0 + q_ti * P.dstep, ds = P.ds0 + q_tj * P.dstep;
      const int tdelta = ((dr * P.WA + ds) * P.CA + q_chb) * EB;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const uint32_t poison = (uint32_t)__builtin_amdgcn_sbfe((int)a_inv[h][i], (unsigned)tap, 1u) |
                                (valid ? 0u : 0xffffffffu);
        glds16(ra, dst + i * 1024, (uint32_t)(a_base[h][i] + tdelta) | poison);
      }
    } else {
      const int tbo = ((P.tr0 + q_ti * P.tstep) * P.S + (P.ts0 + q_tj * P.tstep)) * P.CA + q_chb;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const uint32_t off = (valid && b_row[h][i] >= 0) ? (uint32_t)((b_row[h][i] + tbo) * EB + b_c[h][i] * 16) : OOB;
        glds16(rb, dst + i * 1024, off);
      }
    }
  };

  const int wm = wid % WM, wn = wid / WM;
  const int fr = lane & 15, fq = lane >> 4;
  v4f acc[2 * TMQ][2 * TNQ];
#pragma unroll
  for (int i = 0; i < 2 * TMQ; ++i)
#pragma unroll
    for (int j = 0; j < 2 * TNQ; ++j) acc[i][j] = v4f{0.f, 0.f, 0.f, 0.f};

  // prologue: steps 0 and 1, every quarter in consumption order (X0, W0, W1, X1)
#pragma unroll
  for (int st = 0; st < 2; ++st) {
    issue(0, 0, st); issue(1, 0, st); issue(1, 1, st); issue(0, 1, st);
    advance();
  }
  // fragments: X rows of this wave in a half = wm*HX + i*16 + fr; W rows = wn*HW + j*16 + fr.
  // A fragment holds the two 16-B chunks this lane feeds to one K-step's MFMAs: bf16 -- chunk fq
  // (k-sub-step 0) and 4 + fq (k-sub-step 1); fp8 -- chunks 2fq, 2fq+1 of the 16x16x128 operand
  auto read_frag = [&](const char* base, int row, v4i (&f)[2]) {
    if constexpr (OP == OP_BF16) {
      f[0] = *reinterpret_cast<const v4i*>(base + swz128(row, fq));
      f[1] = *reinterpret_cast<const v4i*>(base + swz128(row, 4 + fq));
    } else {
      f[0] = *reinterpret_cast<const v4i*>(base + swz128(row, 2 * fq));
      f[1] = *reinterpret_cast<const v4i*>(base + swz128(row, 2 * fq + 1));
    }
  };
  auto read_x = [&](const char* base, v4i (&f)[TMQ][2]) {
#pragma unroll
    for (int i = 0; i < TMQ; ++i) read_frag(base, wm * HX + i * 16 + fr, f[i]);
  };
  auto read_w = [&](const char* base, v4i (&f)[TNQ][2]) {
#pragma unroll
    for (int j = 0; j < TNQ; ++j) read_frag(base, wn * HW + j * 16 + fr, f[j]);
  };
  auto mma = [&](int i0, int j0, const v4i (&xf)[TMQ][2], const v4i (&wf)[TNQ][2]) {
    __builtin_amdgcn_s_setprio(1);
    if constexpr (OP == OP_BF16) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int i = 0; i < TMQ; ++i)
#pragma unroll
          for (int j = 0; j < TNQ; ++j) acc[i0 + i][j0 + j] = mfma16(wf[j][ks], xf[i][ks], acc[i0 + i][j0 + j]);
    } else {
#pragma unroll
      for (int i = 0; i < TMQ; ++i)
#pragma unroll
        for (int j = 0; j < TNQ; ++j) {
          const v8i a8 = __builtin_shufflevector(wf[j][0], wf[j][1], 0, 1, 2, 3, 4, 5, 6, 7);
          const v8i b8 = __builtin_shufflevector(xf[i][0], xf[i][1], 0, 1, 2, 3, 4, 5, 6, 7);
          acc[i0 + i][j0 + j] = mfma_f8<OP>(a8, b8, acc[i0 + i][j0 + j]);
        }
    }
    __builtin_amdgcn_s_setprio(0);
  };

  v4i x0[TMQ][2], x1[TMQ][2], w0f[TNQ][2], w1f[TNQ][2];
  for (int s = 0; s < nk; ++s) {
    const int st = s & 1;
    const char* base = smem + st * STAGE;
    // P0: Q(0,0)
    wait_vm<12>();
    lds_barrier_rd();
    read_x(base, x0);
    read_w(base + 2 * QX, w0f);
    mma(0, 0, x0, w0f);
    // P1: Q(0,1); X0 and W0 of this stage are dead -> refill with step s+2
    wait_vm<10>();
    lds_barrier_rd();
    issue(0, 0, st);
    issue(1, 0, st);
    read_w(base + 2 * QX + QW, w1f);
    mma(0, TNQ, x0, w1f);
    // P2: Q(1,0); W1 dead
    wait_vm<12>();
    lds_barrier_rd();
    issue(1, 1, st);
    read_x(base + QX, x1);
    mma(TMQ, 0, x1, w0f);
    // P3: Q(1,1) from registers; X1 dead
    lds_barrier_rd();
    issue(0, 1, st);
    advance();
    mma(TMQ, TNQ, x1, w1f);
  }
  wait_vm<0>();
  lds_barrier_rd();  // every DMA landed and every fragment read done before the epilogue reuses LDS
  nt_epilogue<CFG, WM, WN, 2 * TMQ, 2 * TNQ, EPI, OP>(P, acc, smem, m0, n0, tmi);
}

// ============================================================================
//          TN implicit GEMM with fp8 operands (wgrad on the MX-rate MFMA)
// ============================================================================
// dW[Kout][R*S*C] += sum over pixels m of dy8[m][kout] (e5m2) * im2col(x8)[m][(tap, c)] (e4m3), times
// the two operands' dequantization factors (device scalars: delayed per-tensor scaling).  A K-step
// is 128 pixels = the K of ONE v_mfma_scale_f32_16x16x128_f8f6f4 (unit block scales), which issues
// twice the bf16 FLOP per cycle; a K-step moves the same 128-B operand rows per pixel block as a
// bf16 step of 64 pixels.  Both tiles sit in LDS row-major by pixel; an operand fragment is four
// ds_read_b64_tr_b8 -- lane 2k'+h of 16-lane group g, read r: pixel row 32g + 8r + k', bytes
// 8h..8h+7 of the fragment's 16 columns (the read transposes; profiles/r2_tr_b8_probe.md,
// scripts/probe_f8_tn.hip).  The 16-B chunk of a row is XOR-swizzled (swz_f8) so the 8 rows of a
// 16-lane group hit 8 distinct 4-bank groups and the two groups serviced together disjoint halves.
// Split-K with fp32 atomics only (deterministic runs keep the bf16 slab path).
struct TnF8Args {
  const uint8_t* dy;   // [Mred][Kout] e5m2
  const uint8_t* x;    // [N][H][W][C] e4m3
  const float* dy_deq; // device scalars: real value = code * deq
  const float* x_deq;
  float* out;          // dW [Kout][Ncols] fp32 (atomic accumulation)
  uint32_t dy_bytes, x_bytes;
  int Mred, Kout, Ncols;
  int H, W, C, S, stride, pad, stride_w;
  FastDiv div_hw, div_w;
  int HoWo, Wo, Ho;
  int steps_per_split, nsteps;
  int adv_r, adv_qh, adv_qn;  // 128 reduction rows = (adv_qn images, adv_qh output rows, adv_r columns)
};

template <int ROWB>
__device__ __forceinline__ int swz_f8(int row) {
  if constexpr (ROWB == 128) return (row & 7) ^ ((row >> 5) & 1);
  else return ((row >> 2) & 1) | (((row >> 5) & 1) << 1);  // 64-B rows: 4 chunks
}

typedef int v2i_t __attribute__((ext_vector_type(2)));

template <int ROWB>
__device__ __forceinline__ v8i frag_tr8(const char* tile, int lane, int chunk) {
  const int g = lane >> 4, kk = (lane & 15) >> 1, h = lane & 1;
  v8i f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = 32 * g + 8 * r + kk;
    const char* p = tile + row * ROWB + ((chunk ^ swz_f8<ROWB>(row)) << 4) + 8 * h;
    const v2i_t v = __builtin_amdgcn_ds_read_tr8_b64_v2i32(
        (__attribute__((address_space(3))) v2i_t*)(reinterpret_cast<uintptr_t>(p)));
    f[2 * r] = v.x;
    f[2 * r + 1] = v.y;
  }
  return f;
}

template <int BMG, bool PW>
__global__ void __launch_bounds__(256, 2) igemm_tn_f8_kernel(const TnF8Args P) {
  constexpr int A_ROWB = BMG, B_ROWB = 128;    // bytes per pixel row of the dy / x tiles
  constexpr int KS = 128;                      // pixels per K-step
  constexpr int A_BYTES = KS * A_ROWB, B_BYTES = KS * B_ROWB, STAGE = A_BYTES + B_BYTES;
  constexpr int WAVES = 4;
  constexpr int A_LPR = A_ROWB / 16, A_RPI = 64 / A_LPR;  // one 1-KiB DMA instruction: A_RPI rows
  constexpr int A_PW = A_BYTES / 1024 / WAVES, B_PW = B_BYTES / 1024 / WAVES;
  constexpr int TM = BMG / 32, TN = 4;         // 2 x 2 waves of (BMG/2) x 64
  static_assert(A_PW * 1024 * WAVES == A_BYTES && B_PW * 1024 * WAVES == B_BYTES, "tile DMA split");
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int ntn = (P.Ncols + 127) / 128;
  const int ntm = (P.Kout + BMG - 1) / BMG;
  const int tiles = ntm * ntn;
  const int lid = xcd_remap(blockIdx.x, (int)gridDim.x);
  const int split = lid / tiles;
  const int bid = lid - split * tiles;
  const int tmi = bid / ntn, tni = bid - (bid / ntn) * ntn;
  const int k0 = tmi * BMG, c0 = tni * 128;
  const int s_begin = split * P.steps_per_split;
  const int s_end = min(P.nsteps, s_begin + P.steps_per_split);

  const int t = threadIdx.x;
  const int lane = t & 63, wid = __builtin_amdgcn_readfirstlane(t >> 6);
  // LDS-DMA as asm (igemm_common.h glds16_asm): with the builtin, hipcc drained the prefetched
  // K-step with an s_waitcnt vmcnt(0) in front of every ds_read_tr8 of the current one
  const v4i rdy = rsrc_words(P.dy, P.dy_bytes);
  const v4i rx = rsrc_words(P.x, P.x_bytes);
  const uint32_t sbase = lds_addr(smem);

  // A (dy) lanes: row within the step, source chunk (kout block of 16) that lands in LDS slot
  int a_lane[A_PW];
#pragma unroll
  for (int i = 0; i < A_PW; ++i) {
    const int arow = (wid * A_PW + i) * A_RPI + lane / A_LPR;
    const int chk = (lane % A_LPR) ^ swz_f8<A_ROWB>(arow);
    const int acol = k0 + chk * 16;
    a_lane[i] = acol < P.Kout ? arow * P.Kout + acol : (int)OOB;
  }
  // B (x) lanes: 8 rows of 128 B per instruction; a 16-B chunk is 16 channels of one tap (C % 16 == 0)
  int brow[B_PW], b_dh[B_PW], b_dw[B_PW], b_chb[B_PW];
#pragma unroll
  for (int i = 0; i < B_PW; ++i) {
    brow[i] = (wid * B_PW + i) * 8 + (lane >> 3);
    const int chk = (lane & 7) ^ swz_f8<B_ROWB>(brow[i]);
    const int col = c0 + chk * 16;
    const int tap = col / P.C;
    b_chb[i] = col < P.Ncols ? col - tap * P.C : (int)OOB;
    const int r = tap / P.S;
    b_dh[i] = r - P.pad;
    b_dw[i] = (tap - r * P.S) - P.pad;
  }
  const uint32_t WC = (uint32_t)(P.W * P.C), HWC = (uint32_t)P.H * WC;
  uint32_t b_n[B_PW], b_ho[B_PW], b_wo[B_PW];
  if constexpr (!PW) {
#pragma unroll
    for (int i = 0; i < B_PW; ++i) {
      const uint32_t m = (uint32_t)(s_begin * KS + brow[i]);
      b_n[i] = fdiv(m, P.div_hw);
      const uint32_t rem = m - b_n[i] * (uint32_t)P.HoWo;
      b_ho[i] = fdiv(rem, P.div_w);
      b_wo[i] = rem - b_ho[i] * (uint32_t)P.Wo;
    }
  }

  auto issue = [&](int step, int buf) {
    const uint32_t As = sbase + buf * STAGE;
    const uint32_t Bs = As + A_BYTES;
    const int mb = step * KS;
    const int abase = mb * P.Kout;
#pragma unroll
    for (int i = 0; i < A_PW; ++i) glds16_asm(rdy, As + (wid * A_PW + i) * 1024, (uint32_t)(abase + a_lane[i]));
#pragma unroll
    for (int i = 0; i < B_PW; ++i) {
      uint32_t off;
      if constexpr (PW) {
        off = (uint32_t)((mb + brow[i]) * P.C + b_chb[i]);  // rows past Mred fall past the buffer
      } else {
        const uint32_t h = __umul24(b_ho[i], (uint32_t)P.stride) + (uint32_t)b_dh[i];
        const uint32_t w = __umul24(b_wo[i], (uint32_t)P.stride_w) + (uint32_t)b_dw[i];
        const bool ok = h < (uint32_t)P.H && w < (uint32_t)P.W;
        const uint32_t o = __umul24(b_n[i], HWC) + __umul24(h, WC) + __umul24(w, (uint32_t)P.C) + (uint32_t)b_chb[i];
        off = ok ? o : OOB;
        uint32_t wo = b_wo[i] + (uint32_t)P.adv_r;
        const uint32_t c1 = wo >= (uint32_t)P.Wo ? 1u : 0u;
        b_wo[i] = c1 ? wo - (uint32_t)P.Wo : wo;
        uint32_t ho = b_ho[i] + (uint32_t)P.adv_qh + c1;
        const uint32_t c2 = ho >= (uint32_t)P.Ho ? 1u : 0u;
        b_ho[i] = c2 ? ho - (uint32_t)P.Ho : ho;
        b_n[i] += (uint32_t)P.adv_qn + c2;
      }
      glds16_asm(rx, Bs + (wid * B_PW + i) * 1024, off);
    }
  };

  const int wm = wid & 1, wn = wid >> 1;
  v4f acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = v4f{0.f, 0.f, 0.f, 0.f};

  constexpr int LPS = A_PW + B_PW;
  const int nst = s_end - s_begin;
  if (nst > 0) issue(s_begin, 0);
  wait_vm<0>();
  lds_barrier();
  for (int i = 0; i < nst; ++i) {
    const int cur = i & 1;
    if (i + 1 < nst) issue(s_begin + i + 1, cur ^ 1);
    const char* As = smem + cur * STAGE;
    const char* Bs = As + A_BYTES;
    v8i af[TM], bfr[TN];
#pragma unroll
    for (int m = 0; m < TM; ++m) af[m] = frag_tr8<A_ROWB>(As, lane, wm * TM + m);
#pragma unroll
    for (int j = 0; j < TN; ++j) bfr[j] = frag_tr8<B_ROWB>(Bs, lane, wn * TN + j);
#pragma unroll
    for (int m = 0; m < TM; ++m)
#pragma unroll
      for (int j = 0; j < TN; ++j)  // A = dy (e5m2: cbsz 1), B = x (e4m3: blgp 0), unit block scales
        acc[m][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af[m], bfr[j], acc[m][j], 1, 0, 0, 0, 0, 0);
    if (i + 1 < nst) wait_vm<0>();
    lds_barrier_rd();  // this step's fragment reads retired before the next refill of its buffer
  }
  (void)LPS;

  // epilogue: lane (fq, fr) holds kout rows fq*4+e, column fr of each fragment; dequantize, then one
  // 256-B row segment per atomic wave-instruction through a wave-private LDS image (the drained
  // pipeline buffers), as the bf16 TN epilogue
  const float sc = P.dy_deq[0] * P.x_deq[0];
  const int fq = lane >> 4, fr = lane & 15;
  float* stg = reinterpret_cast<float*>(smem) + wid * (TM * 16) * 64;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = i * 16 + fq * 4 + e;
        stg[r * 64 + ((j * 16 + fr) ^ (((r >> 2) & 1) << 4))] = acc[i][j][e] * sc;
      }
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the region is wave-private
  __builtin_amdgcn_wave_barrier();
  const int col = c0 + wn * 64 + lane;
  const int row0 = k0 + wm * TM * 16;
  if (col < P.Ncols) {
#pragma unroll 8
    for (int r = 0; r < TM * 16; ++r) {
      const float v = stg[r * 64 + (lane ^ (((r >> 2) & 1) << 4))];
      if (row0 + r < P.Kout) unsafeAtomicAdd(P.out + (int64_t)(row0 + r) * P.Ncols + col, v);
    }
  }
}

// ============================================================================
//                                   host side
// ============================================================================
// The NT workgroup tiles: the one place a (BM, BN) pair meets its template arguments.  WM x WN
// waves of TM x TN MFMA tiles (plain and halo kernels), the depth of the tile's K32 ring, whether
// its 2-stage K64 kernels (plain, fp8, halo) exist, and the wave grid of its quadrant-phased kernel
// (0: none).  plan_nt() chooses among them; dispatch_nt() instantiates from the tag.
template <int WM_, int WN_, int TM_, int TN_, int RING_, bool K64_ = true, int QWM_ = 0, int QWN_ = 0>
struct NtTile {
  static constexpr int WM = WM_, WN = WN_, TM = TM_, TN = TN_, RING = RING_, QWM = QWM_, QWN = QWN_;
  static constexpr bool K64 = K64_;
  static constexpr int BM = WM * TM * 16, BN = WN * TN * 16;
  static constexpr int TMQ = QWM ? BM / (QWM * 32) : 0, TNQ = QWN ? BN / (QWN * 32) : 0;  // NtqCfg
};
constexpr int nt_tile_key(int bm, int bn) { return bm * 1024 + bn; }
template <class F>
static void with_nt_tile(int bm, int bn, F&& f) {
  switch (nt_tile_key(bm, bn)) {
    case nt_tile_key(256, 64): return f(NtTile<4, 1, 4, 4, 4>{});
    case nt_tile_key(64, 128): return f(NtTile<2, 2, 2, 4, 4>{});
    case nt_tile_key(128, 128): return f(NtTile<2, 2, 4, 4, 4, true, 2, 2>{});  // 64 KB, two blocks per CU
    case nt_tile_key(128, 256): return f(NtTile<2, 2, 4, 8, 3, false>{});       // 72 KB, two blocks per CU
    case nt_tile_key(256, 256): return f(NtTile<4, 2, 4, 8, 5, true, 2, 4>{});  // 8 waves, 160 KB ring
  }
  throw std::logic_error("no NT tile " + std::to_string(bm) + "x" + std::to_string(bn));
}

template <class T, int STAGES, bool C64, int EPI, int OP = OP_BF16, bool K32 = false>
static void run_nt(const NtArgs& a, hipStream_t st) {
  using CFG = NtCfg<T::WM, T::WN, T::TM, T::TN, STAGES, K32>;
  const int ntm = ceil_div(a.M, CFG::BM), ntn = ceil_div(a.Nout, CFG::BN);
  // a K loop shorter than the pipeline never touches the last buffers: request only the LDS it
  // uses so more blocks fit per CU (the short-K 1x1 convs are bound by their epilogue stores)
  constexpr int KE = OP == OP_BF16 ? (K32 ? 32 : 64) : 128;
  const int nk = C64 ? a.ntaps * (a.CA / KE) : (a.Kg + KE - 1) / KE;
  const int smem = std::max(std::max(1, std::min(nk, STAGES)) * CFG::STAGE_BYTES, CFG::EPI_BYTES);
  launch_lds<igemm_nt_kernel<T::WM, T::WN, T::TM, T::TN, STAGES, C64, EPI, OP, false, K32>>(
      "igemm_nt", ntm * ntn, CFG::NT, CFG::SMEM, smem, st, a);
}

// The quadrant-phased kernel (igemm_ntq_kernel) runs the bf16 256x256 and 128x128 C64 tiles (r4ab,
// interleaved: 18.86 / 18.85 ms vs 18.93 / 18.92 / 18.97 on the 256x256 tile alone).  Measured and
// removed in round 5 (git history: 242a23b): the ping-pong 256x256 kernel (won isolated GEMMs, lost
// ~0.1 ms in the step), the read-ahead NTQ loop, stream-K for sub-wave grids (owners spun beside
// the side-stream wgrads: 40 vs 19 ms/step) and the fp8 quadrant-phased tile.
template <class T, int EPI>
static void run_ntq(const NtArgs& a, hipStream_t st) {
  using Q = NtqCfg<T::QWM, T::QWN, T::TMQ, T::TNQ>;
  static_assert(Q::BM == T::BM && Q::BN == T::BN, "quadrant-phased geometry of the tile");
  const int ntm = ceil_div(a.M, Q::BM), ntn = ceil_div(a.Nout, Q::BN);
  launch_lds<igemm_ntq_kernel<T::QWM, T::QWN, T::TMQ, T::TNQ, EPI, OP_BF16>>(
      "igemm_ntq", ntm * ntn, Q::NT, Q::SMEM, Q::SMEM, st, a);
}

template <class T, int EPI>
static void run_nt_halo(const NtArgs& a, hipStream_t st) {
  using CFG = NtCfg<T::WM, T::WN, T::TM, T::TN, 2>;
  const int ntm = ceil_div(a.M, CFG::BM), ntn = ceil_div(a.Nout, CFG::BN);
  const int smem = std::max((int)(a.halo_nbuf * a.halo_bytes) + 2 * CFG::BN * 128 + 128, CFG::EPI_BYTES);
  launch_lds<igemm_nt_kernel<T::WM, T::WN, T::TM, T::TN, 2, true, EPI, OP_BF16, true>>(
      "igemm_nt_halo", ntm * ntn, CFG::NT, 160 * 1024, smem, st, a);
}

// ---------------------------------------------------------------- NT launch plan
// Every NT launch is planned once, by plan_nt(): the introspection (conv_nt_tile), the BN
// partial-buffer sizes (conv_nt_group_rows), the halo sizing and the dispatcher all read the NtPlan
// record, so they cannot disagree.  A new tile is added to plan_nt() (and gets its NtTile row).
constexpr int NT_PLAIN = 0;  // igemm_nt_kernel, per-tap A tiles
constexpr int NT_QUAD = 1;   // igemm_ntq_kernel, quadrant-phased
constexpr int NT_HALO = 2;   // igemm_nt_kernel, A staged once as the halo of the tile's image rows
struct NtQuery {
  int M, Nout, kg_bytes;  // GEMM rows and columns, bytes of a B row
  int op = OP_BF16;       // operand type
  bool c64 = true;        // C64 loader (whole 128-byte K-steps per tap), else the generic one
  bool c8 = false;        // generic loader on the stem's 8-channel source
  int epi = EPI_PLAIN;
  bool halo = false;      // the conv has the halo shape (halo_shape(), bf16 C64 only)
};
struct NtPlan {
  int family;  // NT_PLAIN / NT_QUAD / NT_HALO
  int bm, bn;  // the tile that runs; bm is also the row group of the epilogues' BN partials
  bool k32;    // K32 ring (NT_PLAIN, bf16) instead of the 2-stage K64 main loop
  int stages;
};

// Test hook (conv_nt_force): pin the K32 / K64 main loop of every NT launch, or disable the
// 128x256 short-K tile or the 256x256 tile, so tests can compare the policy's alternatives bit
// for bit.  -1: policy.
static int g_force_k32 = -1, g_force_mid = -1, g_force_wide = -1;
void conv_nt_force(int k32, int mid, int wide) { g_force_k32 = k32; g_force_mid = mid; g_force_wide = wide; }

// K-step per NT launch: K32 ring (4 stages; 5 on the 8-wave tile, 160 KB) or K64 double buffer.
// Measured on MI355X (r2x, bench_conv.py, batch 256): the K32 ring's earlier first MFMA and
// deeper prefetch pay on the huge-M, short-K layer1 GEMMs -- forward 64->256 1x1 136 -> 120 us,
// 256->64 117 -> 103, and the 64-channel dgrads -- while every long-K conv loses 5-20% to the
// doubled barriers and fragment-read restarts (256x14x14 3x3 68 -> 79 us).  Policy: K32 for
// M >= 786432 on forward (stats epilogue) GEMMs and 64-column dgrads.
static bool nt_k32(const NtQuery& q) {
  if (g_force_k32 >= 0) return g_force_k32 == 1;
  return q.M >= 786432 && (q.epi == EPI_STATS || q.Nout <= 64);
}

// Tile policy.  Per K-step a BMxBN tile issues (BM+BN)/8 1-KiB LDS-DMA instructions and reads
// (TM+TN)/(TM*TN) KiB of LDS fragments per MFMA; the 256x256 tile (8 waves of 64x128) halves the
// DMA issues and cuts fragment reads by a quarter per MFMA, but runs one block per CU, so it only
// pays with enough blocks (>= 196, measured on the ResNet-50 shape classes: +10-20% on the 28x28
// and 14x14 layers, -40% on 7x7 with 98 blocks) and a K loop longer than one step.
static bool use_wide_tile(int M, int Nout, int kg_bytes) {
  if (Nout < 256 || g_force_wide == 0) return false;
  const int64_t blocks = (int64_t)((M + 255) / 256) * ((Nout + 255) / 256);
  return kg_bytes >= 256 && blocks >= 196;
}

// Short-K GEMMs with Nout % 256 == 0 (the 1x1 convs' K <= 512 elements): a 4-wave 128x256
// tile (waves of 64x128, the 256x256 tile's wave shape) on the K32 ring, so its LDS (72 KB) lets
// TWO blocks share a CU: one block's epilogue stores overlap the other's loads and MFMAs.  The
// 8-wave 256x256 tile holds a CU alone, and its phases (load, MFMA, store) run back to back:
// PDT_NT_TIMING measured ~45 % of a 256x256 short-K tile in the store phase while HBM idles in
// the load/MFMA phases.  Measured on MI355X (r3j, one box, batch 256): ResNet-50 step 19.24 ms
// (off) -> 18.94 (K <= 512) / 18.95 (K <= 256) / 19.06 (K <= 1024); isolated fwd 4.22 -> 4.16 ms,
// BN-fused dgrad 5.65 -> 5.52 ms.
static bool use_mid_tile(int M, int Nout, int kg_bytes) {
  if (g_force_mid == 0) return false;
  constexpr int kmax = 512;
  return M > 8192 && Nout % 256 == 0 && kg_bytes <= 2 * kmax;
}

static NtPlan plan_nt(const NtQuery& q) {
  NtPlan p{};
  const bool bf16 = q.op == OP_BF16;
  const bool halo = q.halo && bf16 && q.c64;
  const bool k32ok = q.c64 || !q.c8;  // the 8-channel (stem) loader packs 8 taps per K64 step
  // Tile: output channels <= 64 -> tall 256x64 (more M rows per block).  Small M -> short 64x128
  // (enough blocks) -- unless the 256x256 grid alone fills the chip: a 4096^3 GEMM (M = 4096) ran
  // the 64x128 tile at 642 TF/s.  Short K with Nout % 256 == 0 -> 128x256 (use_mid_tile); big
  // GEMMs -> 256x256 (use_wide_tile), else 128x128.
  const bool wide = use_wide_tile(q.M, q.Nout, q.kg_bytes);
  if (q.Nout <= 64) { p.bm = 256; p.bn = 64; }
  else if (q.M <= 8192 && !wide) { p.bm = 64; p.bn = 128; }
  else if (use_mid_tile(q.M, q.Nout, q.kg_bytes)) { p.bm = 128; p.bn = 256; }
  else if (wide) { p.bm = 256; p.bn = 256; }
  else { p.bm = 128; p.bn = 128; }
  // The 128x256 tile exists as the bf16 per-tap K32 kernel only (fewer instantiations): fp8
  // operands, halo staging and the stem's 8-channel loader run 128x128 where the rule above says
  // 128x256 -- the same 128-row groups, so the BN partial buffers are the same either way.
  if (p.bm == 128 && p.bn == 256 && (!bf16 || halo || !k32ok)) p.bn = 128;
  const bool mid = p.bm == 128 && p.bn == 256;
  if (halo) p.family = NT_HALO;
  else if (bf16 && q.c64 && p.bm == p.bn) p.family = NT_QUAD;  // 256x256 and 128x128
  else p.family = NT_PLAIN;
  // fp8 runs the 2-stage pipeline only (fewer instantiations); the 128x256 tile is always K32
  p.k32 = p.family == NT_PLAIN && bf16 && (mid || (k32ok && nt_k32(q)));
  with_nt_tile(p.bm, p.bn, [&](auto tile) { p.stages = p.k32 ? decltype(tile)::RING : 2; });
  return p;
}

int conv_nt_group_rows(int M, int Nout, int kg_bytes) { return plan_nt({M, Nout, kg_bytes}).bm; }

void conv_nt_tile(int M, int Nout, int kg_bytes, int* bm, int* bn) {
  const NtPlan p = plan_nt({M, Nout, kg_bytes});
  *bm = p.bm;
  *bn = p.bn;
}

// Halo staging applies to 3x3 / stride 1 / pad 1 convolutions with a same-size output whose A
// operand has CA = 64 channels (fwd: CA = C, dgrad: CA = K).
// Measured on MI355X (r2p/r2q, bench_conv.py, batch 256): halo staging pays where one channel
// block covers the whole reduction (C = 64, ResNet layer1: fwd 114 -> 103 us, dgrad 111 -> 98,
// BN-fused dgrad 140 -> 130); with several channel blocks the halo reload per block stalls
// (128x28x28: 86 -> 93 us, 512x7x7: 75 -> 88), so those keep the per-tap A tiles.
static bool halo_shape(const ConvShape& s, int CA) {
  return s.R == 3 && s.S == 3 && s.stride == 1 && s.pad == 1 && s.Ho == s.H && s.Wo == s.W && CA == 64;
}

// Fills the halo fields of `a` for the planned tile; false where the halo does not fit in LDS.
static bool setup_halo(NtArgs& a, const NtPlan& p) {
  const int WP = a.WA + 2;
  const int halo_rows = (a.WA + p.bm - 2) / a.WA + 3;
  const int hpix = halo_rows * WP;
  a.halo_bytes = (uint32_t)((hpix + 7) / 8) * 1024;
  a.n_cb = a.CA / 64;
  const int bstage = 2 * p.bn * 128 + 128;
  const bool wide = p.bm == 256 && p.bn == 256;  // 8-wave tile: one block per CU regardless
  const int cap2 = wide ? 160 * 1024 : 80 * 1024;
  if (a.n_cb > 1 && 2 * (int)a.halo_bytes + bstage <= cap2) a.halo_nbuf = 2;
  else if ((int)a.halo_bytes + bstage <= 160 * 1024) a.halo_nbuf = 1;
  else return false;
  a.halo_rows = halo_rows;
  a.div_hw2 = make_fastdiv((uint32_t)WP);
  a.div_ha = make_fastdiv((uint32_t)a.HA);
  return true;
}

// Plan the launch and map the plan to its instantiation.  `halo`: the conv has the halo shape.
template <bool C64, int EPI, int OP = OP_BF16>
static void dispatch_nt(NtArgs& a, bool halo, hipStream_t st) {
  NtQuery q{a.M, a.Nout, a.Kg * (OP == OP_BF16 ? 2 : 1), OP, C64, a.c8 != 0, EPI, halo};
  NtPlan p = plan_nt(q);
  if (p.family == NT_HALO && !setup_halo(a, p)) {  // too wide an image: per-tap A tiles
    q.halo = false;
    p = plan_nt(q);
  }
  with_nt_tile(p.bm, p.bn, [&](auto tile) {
    using T = decltype(tile);
    if constexpr (C64 && OP == OP_BF16) {
      if (p.family == NT_HALO) {
        if constexpr (T::K64) return run_nt_halo<T, EPI>(a, st);
      } else if (p.family == NT_QUAD) {
        if constexpr (T::QWM > 0) return run_ntq<T, EPI>(a, st);
      }
    }
    // (the operand type is tested at run time: an fp8 dispatcher goes on instantiating the bf16
    // kernels of its loader and epilogue, as it always has, so the code object keeps its kernels)
    if (p.family == NT_PLAIN && q.op != OP_BF16) {
      if constexpr (T::K64) return run_nt<T, 2, C64, EPI, OP>(a, st);
    } else if (p.family == NT_PLAIN && p.k32) {
      return run_nt<T, T::RING, C64, EPI, OP_BF16, true>(a, st);
    } else if (p.family == NT_PLAIN) {
      if constexpr (T::K64) return run_nt<T, 2, C64, EPI, OP_BF16>(a, st);
    }
    throw std::logic_error("dispatch_nt: no kernel for the planned launch");
  });
}

static void fill_common(NtArgs& a, int Mi, int Mj) {
  a.Mij = Mi * Mj;
  a.Mj = Mj;
  a.div_ij = make_fastdiv((uint32_t)a.Mij);
  a.div_j = make_fastdiv((uint32_t)Mj);
  a.div_ca = make_fastdiv((uint32_t)a.CA);
  a.div_s = make_fastdiv((uint32_t)a.S);
}

template <int OP>
static void conv_fwd_impl(const void* x, const void* w, const float* oscale, const float* ascale, uint16_t* y,
                          float* part, const ConvShape& s, hipStream_t st, const BnFwdFuse* bn) {
  constexpr int EB = OP == OP_BF16 ? 2 : 1;
  NtArgs a{};
  a.a = reinterpret_cast<const uint16_t*>(x); a.b = reinterpret_cast<const uint16_t*>(w);
  a.out = y; a.part = part; a.oscale = oscale; a.ascale = ascale;
  if (bn != nullptr) { a.sacc = bn->acc; a.part = nullptr; }
  a.a_bytes = (uint32_t)((int64_t)s.N * s.H * s.W * s.C * EB);
  a.b_bytes = (uint32_t)((int64_t)s.K * s.R * s.S * s.C * EB);
  a.o_bytes = (uint32_t)((int64_t)s.N * s.Ho * s.Wo * s.K * 2);
  a.HA = s.H; a.WA = s.W; a.CA = s.C;
  a.Nout = s.K; a.Kg = s.R * s.S * s.C; a.S = s.S;
  a.M = s.N * s.Ho * s.Wo;
  fill_common(a, s.Ho, s.Wo);
  a.ash = s.stride; a.asw = s.sw(); a.aoff_h = -s.pad; a.aoff_w = -s.pad;
  a.OH = s.Ho; a.OW = s.Wo; a.osh = 1; a.osw = 1; a.oph = 0; a.opw = 0;
  a.dense = 1;
  a.tnr = s.R; a.tns = s.S; a.ntaps = s.R * s.S;
  a.tr0 = 0; a.ts0 = 0; a.tstep = 1;
  a.dr0 = 0; a.ds0 = 0; a.dstep = 1;
  // C64 loader: input channels fill whole 128-byte K-steps (64 bf16 / 128 fp8), tap validity
  // bitmask per row
  const bool c64 = s.C % (128 / EB) == 0 && s.R * s.S <= 32;
  const bool halo = OP == OP_BF16 && c64 && s.sw() == 1 && halo_shape(s, s.C);
  if (OP == OP_BF16 && !c64 && s.C == 8 && 8 % s.S == 0) {  // the stem's super-pixel image
    a.c8 = 1;
    a.c8_rows = 8 / s.S;
    a.c8_step = a.c8_rows * s.W * 8 * 2;
  }
  if (part || bn) {
    if (c64) dispatch_nt<true, EPI_STATS, OP>(a, halo, st);
    else dispatch_nt<false, EPI_STATS, OP>(a, halo, st);
  } else {
    if (c64) dispatch_nt<true, EPI_PLAIN, OP>(a, halo, st);
    else dispatch_nt<false, EPI_PLAIN, OP>(a, halo, st);
  }
  if (bn != nullptr) launch_bn_finalize_sums(*bn, a.M, s.K, st);
}

void launch_conv_fwd(const uint16_t* x, const uint16_t* w, uint16_t* y, float* part,
                     const ConvShape& s, hipStream_t st, const BnFwdFuse* bn) {
  conv_fwd_impl<OP_BF16>(x, w, nullptr, nullptr, y, part, s, st, bn);
}

void launch_conv_fwd_fp8(const uint8_t* x, const uint8_t* w, const float* oscale, const float* ascale,
                         uint16_t* y, float* part, const ConvShape& s, hipStream_t st, const BnFwdFuse* bn) {
  if (s.C % 16 != 0) throw std::runtime_error("conv_fwd_fp8: input channels must be a multiple of 16");
  conv_fwd_impl<OP_F8_E4M3>(x, w, oscale, ascale, y, part, s, st, bn);
}

static int dgrad_class_rows(const ConvShape& s, int ph, int pw) {
  const int str = s.stride;
  const int Mi = (s.H - ph + str - 1) / str;
  const int Mj = (s.W - pw + str - 1) / str;
  return (Mi <= 0 || Mj <= 0) ? 0 : s.N * Mi * Mj;
}

int conv_dgrad_bn_groups(const ConvShape& s, int elem_bytes, int fold_k) {
  // the B row of the launch this sizes the partials for: a DgradFold appends fold_k elements to it
  // (conv_dgrad_impl: Kg += CA2), and the tile -- so the row group -- depends on its length
  int g = 0;
  for (int ph = 0; ph < s.stride; ++ph)
    for (int pw = 0; pw < s.stride; ++pw) {
      const int M = dgrad_class_rows(s, ph, pw);
      if (M > 0) g += ceil_div(M, conv_nt_group_rows(M, s.C, (s.R * s.S * s.K + fold_k) * elem_bytes));
    }
  return g;
}

template <int OP>
static void conv_dgrad_impl(const void* dy, const void* wt, const float* oscale, const float* ascale,
                            uint16_t* dx, const uint16_t* addend, const ConvShape& s, hipStream_t st,
                            const BnBwdFuse* bn, int addend_sub, const DgradFold* fold = nullptr) {
  if (addend_sub != 0 && addend_sub != 2) throw std::runtime_error("conv_dgrad: addend_sub must be 0 or 2");
  if (fold != nullptr && (OP != OP_BF16 || s.R != 1 || s.S != 1 || s.stride != 1 || s.pad != 0 ||
                          fold->CA2 != s.C || s.C % 64 != 0 || s.K % 64 != 0))
    throw std::runtime_error("conv_dgrad: the folded BN backward needs a bf16 1x1 / stride-1 conv, 64-channel multiples");
  constexpr int EB = OP == OP_BF16 ? 2 : 1;
  const int str = s.stride;
  // full: dy rows are whole 128-byte K-steps per tap (the C64 loader, any stride).  fp8 with
  // K % 16 == 0 otherwise (the 64-channel layer-1 convs): the generic loader packs K-steps across
  // taps; its tap walk covers stride 1 only (one parity class, all R x S taps).
  const bool full = s.K % (128 / EB) == 0;
  if (!full && (OP == OP_BF16 || s.K % 16 != 0 || str != 1))
    throw std::runtime_error("conv_dgrad: output channels must fill 128-byte rows (64 bf16 / 128 fp8), "
                             "or be a multiple of 16 for a stride-1 fp8 dgrad");
  int group0 = 0;
  for (int ph = 0; ph < str; ++ph)
    for (int pw = 0; pw < str; ++pw) {
      NtArgs a{};
      a.a = reinterpret_cast<const uint16_t*>(dy); a.b = reinterpret_cast<const uint16_t*>(wt);
      a.out = dx; a.addend = addend; a.part = nullptr; a.oscale = oscale; a.ascale = ascale;
      a.add_sub = addend ? addend_sub : 0;
      a.add_h = addend_sub ? (s.H + 1) / 2 : s.H;
      a.add_w = addend_sub ? (s.W + 1) / 2 : s.W;
      a.add_bytes = (uint32_t)((int64_t)s.N * a.add_h * a.add_w * s.C * 2);
      a.a_bytes = (uint32_t)((int64_t)s.N * s.Ho * s.Wo * s.K * EB);
      a.b_bytes = (uint32_t)((int64_t)s.C * s.R * s.S * s.K * EB);
      a.o_bytes = (uint32_t)((int64_t)s.N * s.H * s.W * s.C * 2);
      a.HA = s.Ho; a.WA = s.Wo; a.CA = s.K;
      a.Nout = s.C; a.Kg = s.R * s.S * s.K; a.S = s.S;
      const int Mi = (s.H - ph + str - 1) / str;
      const int Mj = (s.W - pw + str - 1) / str;
      if (Mi <= 0 || Mj <= 0) continue;
      a.M = s.N * Mi * Mj;
      fill_common(a, Mi, Mj);
      a.ash = 1; a.asw = 1; a.aoff_h = 0; a.aoff_w = 0;
      a.OH = s.H; a.OW = s.W; a.osh = str; a.osw = str; a.oph = ph; a.opw = pw;
      a.dense = (str == 1);
      // taps of this parity class: r = r0 + str*i with (ph + pad - r0) % str == 0, and the
      // dy row it reads is ho = hi + (ph + pad - r)/str = hi + dr0 - i
      const int r0 = (ph + s.pad) % str, s0 = (pw + s.pad) % str;
      a.tnr = r0 < s.R ? (s.R - r0 + str - 1) / str : 0;
      a.tns = s0 < s.S ? (s.S - s0 + str - 1) / str : 0;
      a.ntaps = a.tnr * a.tns;  // 0 -> kernel writes zeros for this class
      const bool halo = OP == OP_BF16 && halo_shape(s, s.K);
      if (a.ntaps > 32) throw std::runtime_error("conv_dgrad: more than 32 taps per parity class");
      a.tr0 = r0; a.ts0 = s0; a.tstep = str;
      a.dr0 = (ph + s.pad - r0) / str; a.ds0 = (pw + s.pad - s0) / str; a.dstep = -1;
      if (fold != nullptr) {  // K-concatenated [dy | z] against B rows [C][K + C] (DgradFold)
        a.a2 = fold->a2; a.CA2 = fold->CA2; a.bias = fold->bias;
        a.a2_bytes = (uint32_t)((int64_t)a.M * fold->CA2 * EB);
        a.Kg += fold->CA2;
        a.b_bytes = (uint32_t)((int64_t)s.C * a.Kg * EB);
      }
      if (bn != nullptr) {
        a.bn_y = bn->y; a.bn_z = bn->z; a.bn_stats = bn->stats; a.bn_part = bn->part; a.bn_acc = bn->acc;
        if (bn->y2 != nullptr) {
          if (bn->acc == nullptr || bn->acc2 == nullptr || bn->stats2 == nullptr || bn->mask != 3 || addend == nullptr)
            throw std::runtime_error("conv_dgrad: the second BN (y2) needs acc mode, its accumulator and "
                                     "statistics, mask 3 and the residual addend");
          a.bn_y2 = bn->y2; a.bn_stats2 = bn->stats2; a.bn_acc2 = bn->acc2;
        }
        a.bn_mask = bn->mask; a.bn_group0 = group0;
        group0 += ceil_div(a.M, conv_nt_group_rows(a.M, a.Nout, a.Kg * EB));
        if constexpr (OP != OP_BF16) {
          if (!full) { dispatch_nt<false, EPI_BNB, OP>(a, halo, st); continue; }
        }
        dispatch_nt<true, EPI_BNB, OP>(a, halo, st);
      } else {
        if constexpr (OP != OP_BF16) {
          if (!full) { dispatch_nt<false, EPI_PLAIN, OP>(a, halo, st); continue; }
        }
        dispatch_nt<true, EPI_PLAIN, OP>(a, halo, st);
      }
    }
}

void launch_conv_dgrad(const uint16_t* dy, const uint16_t* wt, uint16_t* dx, const uint16_t* addend,
                       const ConvShape& s, hipStream_t st, const BnBwdFuse* bn, int addend_sub,
                       const DgradFold* fold) {
  conv_dgrad_impl<OP_BF16>(dy, wt, nullptr, nullptr, dx, addend, s, st, bn, addend_sub, fold);
}

void launch_conv_dgrad_fp8(const uint8_t* dy, const uint8_t* wt, const float* oscale, const float* ascale,
                           uint16_t* dx, const uint16_t* addend, const ConvShape& s, hipStream_t st,
                           const BnBwdFuse* bn, int addend_sub) {
  conv_dgrad_impl<OP_F8_E5M2>(dy, wt, oscale, ascale, dx, addend, s, st, bn, addend_sub);
}

// ------------------------------------------------------------------- wgrad (bf16: wgrad.hip)
// fp8 weight gradient (igemm_tn_f8_kernel): split-K planned like plan_wg (wgrad.hip) with 128-pixel steps
void conv_wgrad_fp8_plan(const ConvShape& s, int out[4]) {
  const int bmg = s.K % 128 == 0 ? 128 : 64;
  const int ncols = s.R * s.S * s.C;
  const int tiles = ((s.K + bmg - 1) / bmg) * ((ncols + 127) / 128);
  const int64_t mred = (int64_t)s.N * s.Ho * s.Wo;
  const int nsteps = (int)((mred + 127) / 128);
  int splits = ((tiles <= 4 ? 2048 : 1024) + tiles - 1) / tiles;
  splits = std::min(splits, std::max(1, nsteps / 8));
  const int64_t dw_bytes = (int64_t)s.K * ncols * 4;
  splits = (int)std::min<int64_t>(splits, std::max<int64_t>(1, ((int64_t)32 << 20) / dw_bytes));
  splits = std::max(1, std::min(splits, 1024));
  const int sps = (nsteps + splits - 1) / splits;
  out[0] = bmg; out[1] = tiles; out[2] = (nsteps + sps - 1) / sps; out[3] = sps;
}

void launch_conv_wgrad_fp8(const uint8_t* dy8, const uint8_t* x8, const float* dy_deq, const float* x_deq,
                           float* dw, const ConvShape& s, bool accumulate, hipStream_t st) {
  if (s.C % 16 != 0 || s.K % 64 != 0) throw std::runtime_error("conv_wgrad_fp8: needs C % 16 == 0, K % 64 == 0");
  int pl[4];
  conv_wgrad_fp8_plan(s, pl);
  TnF8Args a{};
  a.dy = dy8; a.x = x8; a.dy_deq = dy_deq; a.x_deq = x_deq; a.out = dw;
  a.dy_bytes = (uint32_t)((int64_t)s.N * s.Ho * s.Wo * s.K);
  a.x_bytes = (uint32_t)((int64_t)s.N * s.H * s.W * s.C);
  a.Mred = s.N * s.Ho * s.Wo; a.Kout = s.K; a.Ncols = s.R * s.S * s.C;
  a.H = s.H; a.W = s.W; a.C = s.C; a.S = s.S; a.stride = s.stride; a.pad = s.pad; a.stride_w = s.sw();
  a.HoWo = s.Ho * s.Wo; a.Wo = s.Wo; a.Ho = s.Ho;
  a.div_hw = make_fastdiv((uint32_t)a.HoWo);
  a.div_w = make_fastdiv((uint32_t)s.Wo);
  a.nsteps = (a.Mred + 127) / 128;
  a.steps_per_split = pl[3];
  a.adv_r = 128 % s.Wo;
  a.adv_qh = (128 / s.Wo) % s.Ho;
  a.adv_qn = (128 / s.Wo) / s.Ho;
  if (!accumulate) hipMemsetAsync(dw, 0, (size_t)s.K * a.Ncols * sizeof(float), st);
  const bool pw = s.R == 1 && s.S == 1 && s.stride == 1 && s.sw() == 1 && s.pad == 0 && s.H == s.Ho && s.W == s.Wo;
  const int grid = pl[1] * pl[2];
  const int smem = 2 * (128 * pl[0] + 128 * 128);
  // the <BMG, PW> instantiation, selected once
  auto run = [&](auto bmg, auto pwc) {
    launch_lds<igemm_tn_f8_kernel<decltype(bmg)::value, decltype(pwc)::value>>("igemm_tn_f8", grid, 256, smem, smem,
                                                                               st, a);
  };
  auto with_pw = [&](auto bmg) {
    if (pw) run(bmg, std::true_type{});
    else run(bmg, std::false_type{});
  };
  if (pl[0] == 128) with_pw(std::integral_constant<int, 128>{});
  else with_pw(std::integral_constant<int, 64>{});
}

}  // namespace pdt
