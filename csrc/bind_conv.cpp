// Bindings of the layout / packing kernels, the convolutions (bf16 and fp8: forward, dgrad, weight
// gradient) and the stem.
#include "bind_util.h"

using namespace pdt::bind;

namespace {

// ------------------------------------------------------------------ layout
Tensor image_to_nhwc(const Tensor& x) {
  check_cuda(x, "x");
  TORCH_CHECK(x.scalar_type() == at::kFloat && x.dim() == 4, "image must be fp32 NCHW");
  c10::hip::HIPGuard g(x.get_device());
  int N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  int Cp = ((C + 7) / 8) * 8;
  auto y = at::empty({N, H, W, Cp}, x.options().dtype(at::kBFloat16));
  pdt::launch_image_to_nhwc(x.data_ptr<float>(), bf(y), N, C, H, W, Cp, cur_stream(x));
  return y;
}

Tensor pack_weight(const Tensor& w, int64_t cpad) {
  TORCH_CHECK(w.is_cuda() && w.dim() == 4 && w.scalar_type() == at::kFloat, "weight must be fp32 4-D");
  c10::hip::HIPGuard g(w.get_device());
  int K = w.size(0), C = w.size(1), R = w.size(2), S = w.size(3);
  int Cp = std::max<int>((int)cpad, C);
  auto out = at::empty({K, R, S, Cp}, w.options().dtype(at::kBFloat16));
  int64_t st[4] = {w.stride(0), w.stride(1), w.stride(2), w.stride(3)};
  pdt::launch_pack_weight(w.data_ptr<float>(), st, bf(out), K, C, R, S, Cp, cur_stream(w));
  return out;
}

Tensor pack_weight_t(const Tensor& w) {
  TORCH_CHECK(w.is_cuda() && w.dim() == 4 && w.scalar_type() == at::kFloat, "weight must be fp32 4-D");
  c10::hip::HIPGuard g(w.get_device());
  int K = w.size(0), C = w.size(1), R = w.size(2), S = w.size(3);
  auto out = at::empty({C, R, S, K}, w.options().dtype(at::kBFloat16));
  int64_t st[4] = {w.stride(0), w.stride(1), w.stride(2), w.stride(3)};
  pdt::launch_pack_weight_t(w.data_ptr<float>(), st, bf(out), K, C, R, S, cur_stream(w));
  return out;
}

// (wq uint8 e4m3 [K,R,S,Cp], oscale fp32 [K]); act_deq: optional 1-element dequant factor of the
// activation operand, folded into oscale
std::tuple<Tensor, Tensor> pack_weight_fp8(const Tensor& w, int64_t cpad, const std::optional<Tensor>& act_deq) {
  TORCH_CHECK(w.is_cuda() && w.dim() == 4 && w.scalar_type() == at::kFloat, "weight must be fp32 4-D");
  const float* ad = opt(act_deq) ? dev_scalar(*act_deq, "act_deq") : nullptr;
  c10::hip::HIPGuard g(w.get_device());
  int K = w.size(0), C = w.size(1), R = w.size(2), S = w.size(3);
  int Cp = std::max<int>((int)cpad, C);
  auto wq = at::empty({K, R, S, Cp}, w.options().dtype(at::kByte));
  auto osc = at::empty({K}, w.options());
  int64_t st[4] = {w.stride(0), w.stride(1), w.stride(2), w.stride(3)};
  pdt::launch_pack_weight_fp8(w.data_ptr<float>(), st, wq.data_ptr<uint8_t>(), osc.data_ptr<float>(), ad, K,
                              C, R, S, Cp, cur_stream(w));
  return {wq, osc};
}

// flat fp32 -> bf16 mirror (refresh when parameters changed outside the fused SGD step)
void cast_to_bf16(const Tensor& x, Tensor y) {
  check_cuda(x, "x");
  check_cuda(y, "y");
  TORCH_CHECK(x.scalar_type() == at::kFloat && y.scalar_type() == at::kBFloat16 && x.numel() == y.numel(),
              "cast_to_bf16: fp32 -> bf16 of equal size");
  c10::hip::HIPGuard gd(x.get_device());
  pdt::launch_cast_f32_bf16(x.data_ptr<float>(), bf(y), x.numel(), cur_stream(x));
}

// table: int64 [n][4] = (offset, K, C, RS) on the device; src/dst: flat bf16 mirrors
void pack_t_batched(const Tensor& src, Tensor dst, const Tensor& table, int64_t max_tiles) {
  check_cuda(src, "src");
  check_cuda(dst, "dst");
  TORCH_CHECK(table.is_cuda() && table.scalar_type() == at::kByte && table.is_contiguous(),
              "pack_t_batched: table must be a device byte tensor");
  const int64_t eb = (int64_t)pdt::pack_t_entry_bytes();
  TORCH_CHECK(table.numel() % eb == 0, "pack_t_batched: table size");
  c10::hip::HIPGuard gd(src.get_device());
  pdt::launch_pack_t_batched(cbf(src), bf(dst), table.data_ptr(), (int)(table.numel() / eb),
                             (int)max_tiles, cur_stream(src));
}

int64_t pack_t_entry_bytes() { return (int64_t)pdt::pack_t_entry_bytes(); }

// ------------------------------------------------------------ forward conv
// returns (y, part); part is empty when stats == false
std::tuple<Tensor, Tensor> conv_fwd(const Tensor& x, const Tensor& wk, int64_t stride, int64_t pad,
                                    bool stats) {
  c10::hip::HIPGuard g(x.get_device());
  auto [s, y] = conv_fwd_prologue(x, wk, stride, pad, false);
  Tensor part;
  float* pp = nullptr;
  int M = s.N * s.Ho * s.Wo;
  if (stats) {
    int grows = pdt::conv_nt_group_rows(M, s.K, s.R * s.S * s.C * 2);
    int ng = (M + grows - 1) / grows;
    part = at::empty({ng, 2, s.K}, x.options().dtype(at::kFloat));
    pp = part.data_ptr<float>();
  }
  pdt::launch_conv_fwd(cbf(x), cbf(wk), bf(y), pp, s, cur_stream(x));
  return {y, part};
}

// BN finalize inside the conv (kernels.h BnFwdFuse): checks its operands and allocates `stats`
pdt::BnFwdFuse bn_fwd_fuse(const Tensor& x, int K, int64_t count, int64_t M, const Tensor& acc,
                           const Tensor& rm, const Tensor& rv, const Tensor& gamma, const Tensor& beta,
                           double momentum, double eps, Tensor& stats) {
  TORCH_CHECK(M == count, "conv_fwd_bn: count mismatch");
  TORCH_CHECK(acc.scalar_type() == at::kDouble && acc.is_contiguous() && acc.numel() >= pdt::kStatSlots * 2 * K &&
              acc.device() == x.device(), "conv_fwd_bn: acc must be a contiguous fp64 [8][2][K] device tensor");
  TORCH_CHECK(gamma.scalar_type() == at::kFloat && beta.scalar_type() == at::kFloat && gamma.numel() == K,
              "BN params must be fp32 [K]");
  TORCH_CHECK(!rm.defined() || (rm.scalar_type() == at::kFloat && rv.defined() && rm.numel() == K),
              "running stats must be fp32 [K]");
  stats = at::empty({4, K}, x.options().dtype(at::kFloat));
  return pdt::BnFwdFuse{acc.data_ptr<double>(), gamma.data_ptr<float>(), beta.data_ptr<float>(),
                        rm.defined() ? rm.data_ptr<float>() : nullptr, rv.defined() ? rv.data_ptr<float>() : nullptr,
                        stats.data_ptr<float>(), (float)momentum, (float)eps};
}

// Training-mode conv unit forward in ONE host call: conv with BN partial statistics, then the BN
// finalize (batch mean / invstd / scale / shift, running-stat update).  Saves a Python -> C++
// round trip per conv unit (155 per ResNet-152 step) over conv_fwd + bn_finalize.
// acc (fp64 [>= 2K], zero, re-zeroed by the finalize): the conv sums the statistics into it and a
// one-thread-per-channel finalize reads them (kernels.h BnFwdFuse; fp64 atomics, so not bitwise
// run-to-run: callers pass it only outside deterministic mode), else the partials + bn_finalize.
std::tuple<Tensor, Tensor> conv_fwd_bn(const Tensor& x, const Tensor& wk, int64_t stride, int64_t pad,
                                       int64_t count, const Tensor& rm, const Tensor& rv, const Tensor& gamma,
                                       const Tensor& beta, double momentum, double eps,
                                       const std::optional<Tensor>& acc) {
  if (opt(acc)) {
    c10::hip::HIPGuard g(x.get_device());
    auto [s, y] = conv_fwd_prologue(x, wk, stride, pad, false);
    Tensor stats;
    auto f = bn_fwd_fuse(x, s.K, count, (int64_t)s.N * s.Ho * s.Wo, *acc, rm, rv, gamma, beta, momentum, eps,
                         stats);
    pdt::launch_conv_fwd(cbf(x), cbf(wk), bf(y), nullptr, s, cur_stream(x), &f);
    return {y, stats};
  }
  auto yp = conv_fwd(x, wk, stride, pad, true);
  Tensor stats = bn_finalize(std::get<1>(yp), count, rm, rv, gamma, beta, momentum, eps, 0);
  return {std::get<0>(yp), stats};
}

// fp8 forward conv; with `bn` = (count, rm, rv, gamma, beta, momentum, eps, acc) the BN finalize runs
// inside the conv as in conv_fwd_bn, and the second result is the [4][K] statistics, not partials
std::tuple<Tensor, Tensor> conv_fwd_fp8(const Tensor& x, const Tensor& wq, const Tensor& oscale,
                                        int64_t stride, int64_t pad, bool stats,
                                        const std::optional<Tensor>& ascale, const std::optional<py::tuple>& bn) {
  c10::hip::HIPGuard g(x.get_device());
  auto [s, y] = conv_fwd_prologue(x, wq, stride, pad, true);
  TORCH_CHECK(oscale.is_cuda() && oscale.scalar_type() == at::kFloat && oscale.numel() == wq.size(0),
              "oscale must be fp32 [K]");
  const float* asp = opt(ascale) ? dev_scalar(*ascale, "ascale") : nullptr;
  Tensor part;
  float* pp = nullptr;
  int M = s.N * s.Ho * s.Wo;
  std::optional<pdt::BnFwdFuse> fuse;
  if (bn.has_value()) {
    const py::tuple& b = *bn;
    TORCH_CHECK(b.size() == 8, "bn = (count, rm, rv, gamma, beta, momentum, eps, acc)");
    auto maybe = [](const py::handle& h) { return h.is_none() ? Tensor() : h.cast<Tensor>(); };
    fuse = bn_fwd_fuse(x, s.K, b[0].cast<int64_t>(), M, b[7].cast<Tensor>(), maybe(b[1]), maybe(b[2]),
                       b[3].cast<Tensor>(), b[4].cast<Tensor>(), b[5].cast<double>(), b[6].cast<double>(), part);
  } else if (stats) {
    int grows = pdt::conv_nt_group_rows(M, s.K, s.R * s.S * s.C);
    part = at::empty({(M + grows - 1) / grows, 2, s.K}, x.options().dtype(at::kFloat));
    pp = part.data_ptr<float>();
  }
  pdt::launch_conv_fwd_fp8(x.data_ptr<uint8_t>(), wq.data_ptr<uint8_t>(), oscale.data_ptr<float>(), asp,
                           bf(y), pp, s, cur_stream(x), fuse ? &*fuse : nullptr);
  return {y, part};
}

// ------------------------------------------------------------------- dgrad
// wt: optional pre-packed bf16 [C][R][S][K] weights (flat-space dgrad mirror)
Tensor packed_t_or_pack(const Tensor& w, const std::optional<Tensor>& wt_in) {
  const Tensor* wt = opt(wt_in);
  if (!wt) return pack_weight_t(w);
  TORCH_CHECK(wt->scalar_type() == at::kBFloat16 && wt->is_contiguous() && wt->dim() == 4 &&
              wt->size(0) == w.size(1) && wt->size(1) == w.size(2) && wt->size(2) == w.size(3) &&
              wt->size(3) == w.size(0), "wt must be bf16 [C,R,S,K] contiguous");
  return *wt;
}

Tensor conv_dgrad(const Tensor& dy, const Tensor& w, std::vector<int64_t> xs, int64_t stride,
                  int64_t pad, const std::optional<Tensor>& addend, const std::optional<Tensor>& wt_in) {
  auto s = dgrad_prologue(dy, w, xs, stride, pad);
  Addend a = dgrad_addend(addend, s);
  c10::hip::HIPGuard g(dy.get_device());
  Tensor wt = packed_t_or_pack(w, wt_in);
  auto dx = at::empty({s.N, s.H, s.W, s.C}, dy.options());
  pdt::launch_conv_dgrad(cbf(dy), cbf(wt), bf(dx), a.ptr, s, cur_stream(dy), nullptr, a.layout);
  return dx;
}

// optional second BN on the same gradient (kernels.h BnBwdFuse::y2): a downsampling block's
// projection-shortcut BN, reduced by the same epilogue into its own [2][C] accumulator
struct SecondBn {
  std::optional<Tensor> y, stats, acc;
};

inline bool is_f32_dev(const Tensor* t, int64_t numel) {
  return t && t->is_cuda() && t->scalar_type() == at::kFloat && t->is_contiguous() && t->numel() == numel;
}

// Shared body of the dgrads with the BatchNorm backward of the unit that produced x fused into the
// epilogue: `launch(s, dx, addend, bn, stream, addend_layout)` runs the BN-fused dgrad.  Returns
// (g, sums) with g = dx * relu'(unit) (mask 0/1/2 as bn_act_bwd_reduce, 3: the ReLU bitmask) and
// sums[2][C] = (sum g, sum g*(y - mean)); optional dgamma/dbeta accumulate like bn_act_bwd_reduce.
// bn_act_bwd_apply(g, ..., mask=0) then yields that unit's dy.
template <typename Launch>
std::tuple<Tensor, Tensor> dgrad_bn_core(const Tensor& dy_like, const pdt::ConvShape& s,
                                         const std::optional<Tensor>& addend, const Tensor& y,
                                         const std::optional<Tensor>& z_in, const Tensor& stats, int64_t mask,
                                         const std::optional<Tensor>& dgamma,
                                         const std::optional<Tensor>& dbeta, const std::optional<Tensor>& acc_in,
                                         const SecondBn& bn2, Launch&& launch, int fold_k = 0) {
  check_bf16_nhwc(y, "y");
  TORCH_CHECK(y.size(0) == s.N && y.size(1) == s.H && y.size(2) == s.W && y.size(3) == s.C,
              "dgrad_bn: y must have the shape of x");
  check_stats(stats, s.C);
  TORCH_CHECK(mask >= 0 && mask <= 3, "mask must be 0, 1, 2 or 3");
  const Tensor* z = opt(z_in);
  const uint16_t* zp = nullptr;
  if (mask == 1) {
    TORCH_CHECK(z, "mask 1 needs z");
    check_bf16_nhwc(*z, "z");
    TORCH_CHECK(z->sizes() == y.sizes(), "z shape mismatch");
    zp = cbf(*z);
  } else if (mask == 3) {  // ReLU bitmask from bn_act_fwd_mask: one byte per 8 channels
    TORCH_CHECK(z, "mask 3 needs the ReLU bitmask");
    check_cuda(*z, "zmask");
    TORCH_CHECK(z->scalar_type() == at::kByte && z->numel() * 8 == y.numel(), "zmask must be uint8 [numel/8]");
    zp = reinterpret_cast<const uint16_t*>(z->data_ptr());
  }
  Addend a = dgrad_addend(addend, s);
  const Tensor* acc = opt(acc_in);
  const Tensor* y2 = opt(bn2.y);
  TORCH_CHECK(!y2 || acc, "the second BN needs acc mode");
  TORCH_CHECK(!acc || !opt(dgamma), "acc mode: pass dgamma/dbeta to the apply");
  auto pg = bn_param_sinks(dgamma, dbeta, s.C);
  auto dx = at::empty({s.N, s.H, s.W, s.C}, y.options());
  hipStream_t st = cur_stream(dy_like);
  if (acc) {
    // partials fp32-atomically summed by the epilogue into the caller's zeroed [2][C] accumulator:
    // no partial buffer, no reduce launch; the BN parameter gradients are added by the consuming
    // bn_act_bwd_apply(dgamma=, dbeta=), which runs after the sums are complete
    TORCH_CHECK(is_f32_dev(acc, 2 * s.C), "acc must be a contiguous fp32 [2, C] device tensor");
    pdt::BnBwdFuse bn{cbf(y), zp, stats.data_ptr<float>(), nullptr, (int)mask, acc->data_ptr<float>()};
    if (y2) {
      check_bf16_nhwc(*y2, "y2");
      TORCH_CHECK(y2->sizes() == y.sizes(), "y2 must have the shape of y");
      TORCH_CHECK(opt(bn2.stats), "stats2 must be fp32 [4, C]");
      check_stats(*bn2.stats, s.C);
      TORCH_CHECK(is_f32_dev(opt(bn2.acc), 2 * s.C), "acc2 must be a contiguous fp32 [2, C] device tensor");
      TORCH_CHECK(mask == 3 && a.ptr != nullptr, "the second BN needs mask 3 and the residual addend");
      bn.y2 = cbf(*y2);
      bn.stats2 = bn2.stats->data_ptr<float>();
      bn.acc2 = bn2.acc->data_ptr<float>();
    }
    launch(s, bf(dx), a.ptr, &bn, st, a.layout);
    return {dx, acc->view({2, s.C})};
  }
  const int G = pdt::conv_dgrad_bn_groups(s, (int)dy_like.element_size(), fold_k);
  // sums, partials and the reduction workspace as slices of ONE allocation (host issue: each
  // caching-allocator call is ~1-2 us, and this binding runs once per BatchNorm per step)
  const int64_t n_sums = 2 * (int64_t)s.C, n_part = (int64_t)G * 2 * s.C;
  const int64_t n_ws = (int64_t)pdt::bn_bwd_part_ws_floats(G, s.C);
  auto fbuf = at::empty({n_sums + n_part + n_ws}, y.options().dtype(at::kFloat));
  auto sums = fbuf.narrow(0, 0, n_sums).view({2, s.C});
  auto part = fbuf.narrow(0, n_sums, n_part);
  auto ws = fbuf.narrow(0, n_sums + n_part, n_ws);
  pdt::BnBwdFuse bn{cbf(y), zp, stats.data_ptr<float>(), part.data_ptr<float>(), (int)mask};
  launch(s, bf(dx), a.ptr, &bn, st, a.layout);
  pdt::launch_bn_bwd_part_reduce(part.data_ptr<float>(), G, s.C, ws.data_ptr<float>(),
                                 sums.data_ptr<float>(), stats.data_ptr<float>() + s.C, pg.first, pg.second, st);
  return {dx, sums};
}

std::tuple<Tensor, Tensor> conv_dgrad_bn(const Tensor& dy, const Tensor& w, std::vector<int64_t> xs,
                                         int64_t stride, int64_t pad,
                                         const std::optional<Tensor>& addend, const Tensor& y,
                                         const std::optional<Tensor>& z, const Tensor& stats,
                                         int64_t mask, const std::optional<Tensor>& dgamma,
                                         const std::optional<Tensor>& dbeta,
                                         const std::optional<Tensor>& wt_in, const std::optional<Tensor>& acc,
                                         const std::optional<Tensor>& y2, const std::optional<Tensor>& stats2,
                                         const std::optional<Tensor>& acc2) {
  auto s = dgrad_prologue(dy, w, xs, stride, pad);
  c10::hip::HIPGuard g(dy.get_device());
  Tensor wt = packed_t_or_pack(w, wt_in);
  return dgrad_bn_core(dy, s, addend, y, z, stats, mask, dgamma, dbeta, acc, SecondBn{y2, stats2, acc2},
                       [&](const pdt::ConvShape& sh, uint16_t* dx, const uint16_t* ap, const pdt::BnBwdFuse* bn,
                           hipStream_t st, int asub) {
                         pdt::launch_conv_dgrad(cbf(dy), cbf(wt), dx, ap, sh, st, bn, asub);
                       });
}

// BN-fused dgrad of a 1x1 / stride-1 conv with the NEXT unit's BN backward folded in (kernels.h
// DgradFold): dx = [g | z] x wfold^T + bias, then the usual BN-fused epilogue (mask, sums into acc).
// g [N,H,W,K] is that BN's masked gradient, z [N,H,W,C] the conv's input.
std::tuple<Tensor, Tensor> conv_dgrad_bn_fold(const Tensor& g, const Tensor& z_in, const Tensor& wfold,
                                              const Tensor& bias, const Tensor& y, const std::optional<Tensor>& z,
                                              const Tensor& stats, int64_t mask, const std::optional<Tensor>& acc,
                                              const std::optional<Tensor>& dgamma,
                                              const std::optional<Tensor>& dbeta) {
  check_bf16_nhwc(g, "g");
  check_bf16_nhwc(z_in, "z_in");
  const int K = g.size(3), C = z_in.size(3);
  TORCH_CHECK(z_in.size(0) == g.size(0) && z_in.size(1) == g.size(1) && z_in.size(2) == g.size(2),
              "fold: g and z must share N, H, W");
  TORCH_CHECK(wfold.scalar_type() == at::kBFloat16 && wfold.is_contiguous() && wfold.size(0) == C &&
              wfold.size(1) == K + C, "wfold must be bf16 [C][K + C]");
  TORCH_CHECK(bias.scalar_type() == at::kFloat && bias.numel() == C, "bias: fp32 [C]");
  c10::hip::HIPGuard gd(g.get_device());
  auto s = shape_of(g.size(0), g.size(1), g.size(2), C, K, 1, 1, 1, 0);
  pdt::DgradFold fold{cbf(z_in), C, bias.data_ptr<float>()};
  // acc: fp32-atomic BN sums of the unit before (default runs); without it (deterministic runs) the
  // fixed-order partials + reduce path, with that unit's dgamma / dbeta sinks
  return dgrad_bn_core(g, s, std::nullopt, y, z, stats, mask, dgamma, dbeta, acc, SecondBn{},
                       [&](const pdt::ConvShape& sh, uint16_t* dx, const uint16_t* ap, const pdt::BnBwdFuse* bn,
                           hipStream_t st, int asub) {
                         pdt::launch_conv_dgrad(cbf(g), cbf(wfold), dx, ap, sh, st, bn, asub, &fold);
                       },
                       /*fold_k=*/C);  // the partials are sized for the GEMM over K + C
}

// fp8 dgrad operands: dy8 e5m2 NHWC [N,Ho,Wo,K], wt8 e4m3 [C,R,S,K] with per-C scale wscale,
// dy dequant factor ascale (device scalar)
pdt::ConvShape fp8_dgrad_shape(const Tensor& dy8, const Tensor& wt8, const Tensor& wscale, const Tensor& ascale,
                               const std::vector<int64_t>& xs, int64_t stride, int64_t pad) {
  check_u8_nhwc(dy8, "dy8");
  check_cuda(wt8, "wt8");
  TORCH_CHECK(wt8.scalar_type() == at::kByte && wt8.dim() == 4, "wt8 must be uint8 [C,R,S,K]");
  TORCH_CHECK(xs.size() == 4 && xs[3] == wt8.size(0), "dgrad: x channels must equal weight in-channels");
  TORCH_CHECK(wscale.is_cuda() && wscale.scalar_type() == at::kFloat && wscale.numel() == wt8.size(0),
              "wscale must be fp32 [C]");
  dev_scalar(ascale, "ascale");
  auto s = shape_of(xs[0], xs[1], xs[2], xs[3], wt8.size(3), wt8.size(1), wt8.size(2), stride, pad);
  TORCH_CHECK(s.Ho == dy8.size(1) && s.Wo == dy8.size(2) && s.K == dy8.size(3), "dgrad: dy shape mismatch");
  TORCH_CHECK(s.K % 128 == 0 || (s.K % 16 == 0 && s.stride == 1),
              "fp8 dgrad: output channels must be a multiple of 128 (or of 16 at stride 1)");
  return s;
}

Tensor conv_dgrad_fp8(const Tensor& dy8, const Tensor& wt8, const Tensor& wscale, const Tensor& ascale,
                      std::vector<int64_t> xs, int64_t stride, int64_t pad,
                      const std::optional<Tensor>& addend) {
  c10::hip::HIPGuard g(dy8.get_device());
  auto s = fp8_dgrad_shape(dy8, wt8, wscale, ascale, xs, stride, pad);
  Addend a = dgrad_addend(addend, s);
  auto dx = at::empty({s.N, s.H, s.W, s.C}, dy8.options().dtype(at::kBFloat16));
  pdt::launch_conv_dgrad_fp8(dy8.data_ptr<uint8_t>(), wt8.data_ptr<uint8_t>(), wscale.data_ptr<float>(),
                             ascale.data_ptr<float>(), bf(dx), a.ptr, s, cur_stream(dy8), nullptr, a.layout);
  return dx;
}

std::tuple<Tensor, Tensor> conv_dgrad_bn_fp8(const Tensor& dy8, const Tensor& wt8, const Tensor& wscale,
                                             const Tensor& ascale, std::vector<int64_t> xs, int64_t stride,
                                             int64_t pad, const std::optional<Tensor>& addend,
                                             const Tensor& y, const std::optional<Tensor>& z,
                                             const Tensor& stats, int64_t mask,
                                             const std::optional<Tensor>& dgamma,
                                             const std::optional<Tensor>& dbeta,
                                             const std::optional<Tensor>& acc) {
  c10::hip::HIPGuard g(dy8.get_device());
  auto s = fp8_dgrad_shape(dy8, wt8, wscale, ascale, xs, stride, pad);
  return dgrad_bn_core(dy8, s, addend, y, z, stats, mask, dgamma, dbeta, acc, SecondBn{},
                       [&](const pdt::ConvShape& sh, uint16_t* dx, const uint16_t* ap, const pdt::BnBwdFuse* bn,
                           hipStream_t st, int asub) {
                         pdt::launch_conv_dgrad_fp8(dy8.data_ptr<uint8_t>(), wt8.data_ptr<uint8_t>(),
                                                    wscale.data_ptr<float>(), ascale.data_ptr<float>(), dx,
                                                    ap, sh, st, bn, asub);
                       });
}

// --------------------------------------------------------- weight gradient
// the checked operands of a bf16 weight gradient; out: the caller-owned accumulator, if any
struct Wgrad {
  pdt::ConvShape s;
  int C;
  const Tensor* out;
};

Wgrad wgrad_check(const Tensor& dy, const Tensor& x, const std::vector<int64_t>& ws, int64_t stride,
                  int64_t pad, const std::optional<Tensor>& out) {
  check_bf16_nhwc(dy, "dy");
  check_bf16_nhwc(x, "x");
  TORCH_CHECK(ws.size() == 4, "weight shape must be [K,C,R,S]");
  int K = ws[0], C = ws[1], R = ws[2], S = ws[3];
  auto s = shape_of(x.size(0), x.size(1), x.size(2), x.size(3), K, R, S, stride, pad);
  TORCH_CHECK(s.Ho == dy.size(1) && s.Wo == dy.size(2) && K == dy.size(3), "wgrad: dy shape mismatch");
  const Tensor* o = opt(out);
  if (o) {
    TORCH_CHECK(s.C == C, "in-place wgrad needs unpadded input channels");
    check_krsc_out(*o, K, C, R, S);
  }
  return {s, C, o};
}

// dw as an fp32 channels_last tensor of logical shape [K, C, R, S], on the current stream (which
// owns the workspace); zero / zero_n: a buffer the weight-gradient kernel clears (see launch_conv_wgrad)
Tensor wgrad_run(const Tensor& dy, const Tensor& x, const Wgrad& a, bool deterministic, float* zero,
                 int zero_n) {
  const pdt::ConvShape& s = a.s;
  auto fopt = x.options().dtype(at::kFloat);
  size_t wsn = pdt::conv_wgrad_ws_floats(s, deterministic);
  Tensor wsb = wsn ? at::empty({(int64_t)wsn}, fopt) : Tensor();
  Tensor dwp = a.out ? *a.out : at::empty({s.K, s.R, s.S, s.C}, fopt);
  pdt::launch_conv_wgrad(cbf(dy), cbf(x), dwp.data_ptr<float>(), wsn ? wsb.data_ptr<float>() : nullptr, s,
                         deterministic, a.out != nullptr, cur_stream(x), zero, zero_n);
  if (a.out) return dwp;
  Tensor krsc = s.C == a.C ? dwp : dwp.narrow(3, 0, a.C).contiguous();
  return krsc.permute({0, 3, 1, 2});  // [K,C,R,S] view with channels_last strides
}

Tensor conv_wgrad(const Tensor& dy, const Tensor& x, std::vector<int64_t> ws, int64_t stride,
                  int64_t pad, bool deterministic, const std::optional<Tensor>& out) {
  Wgrad a = wgrad_check(dy, x, ws, stride, pad, out);
  c10::hip::HIPGuard g(x.get_device());
  return wgrad_run(dy, x, a, deterministic, nullptr, 0);
}

// conv_wgrad issued on the weight-gradient side stream (SideStream) in one call; dy / x are kept
// for the side stream.
Tensor conv_wgrad_side(int64_t side, const Tensor& dy, const Tensor& x, std::vector<int64_t> ws,
                       int64_t stride, int64_t pad, bool deterministic, const std::optional<Tensor>& out,
                       const std::optional<Tensor>& zero) {
  TORCH_CHECK(side != 0, "conv_wgrad_side: null side stream");
  Wgrad a = wgrad_check(dy, x, ws, stride, pad, out);
  // `zero`: a BN-sum accumulator whose consumer (the apply just queued on the current stream) is
  // done at this point of the side stream: the weight-gradient kernel itself re-zeroes it for its
  // next use (workgroup 0), off the critical path and without a memset launch
  const Tensor* z = opt(zero);
  TORCH_CHECK(!z || (z->scalar_type() == at::kFloat && z->is_contiguous()), "zero: contiguous fp32");
  c10::hip::HIPGuard g(x.get_device());
  SideStream ss(side, (c10::DeviceIndex)x.get_device());
  Tensor r = wgrad_run(dy, x, a, deterministic, z ? z->data_ptr<float>() : nullptr, z ? (int)z->numel() : 0);
  ss.keep({&dy, &x});
  return r;
}

// fp8 weight gradient (conv_igemm.hip igemm_tn_f8_kernel): dy8 e5m2 [N,Ho,Wo,K] and x8 e4m3 [N,H,W,C]
// with their dequantization factors (device fp32 scalars).  Accumulates into `out` (a KRSC-dense fp32
// view, e.g. the flat gradient buffer) or returns a fresh [K,C,R,S] channels_last tensor.  side != 0:
// issued on that stream after the current stream's queued work, like conv_wgrad_side.
Tensor conv_wgrad_fp8(int64_t side, const Tensor& dy8, const Tensor& x8, const Tensor& dy_deq, const Tensor& x_deq,
                      std::vector<int64_t> ws, int64_t stride, int64_t pad, const std::optional<Tensor>& out,
                      const std::optional<Tensor>& zero) {
  TORCH_CHECK(dy8.is_cuda() && x8.is_cuda() && dy8.scalar_type() == at::kByte && x8.scalar_type() == at::kByte &&
              dy8.dim() == 4 && x8.dim() == 4 && dy8.is_contiguous() && x8.is_contiguous(),
              "conv_wgrad_fp8: dy8 / x8 must be contiguous uint8 NHWC device tensors");
  const float* dyq = dev_scalar(dy_deq, "conv_wgrad_fp8: dy_deq");
  const float* xq = dev_scalar(x_deq, "conv_wgrad_fp8: x_deq");
  TORCH_CHECK(ws.size() == 4, "weight shape must be [K,C,R,S]");
  const int K = ws[0], C = ws[1], R = ws[2], S = ws[3];
  TORCH_CHECK(x8.size(3) == C && C % 16 == 0 && K % 64 == 0, "conv_wgrad_fp8: needs C % 16 == 0, K % 64 == 0");
  auto s = shape_of(x8.size(0), x8.size(1), x8.size(2), C, K, R, S, stride, pad);
  TORCH_CHECK(s.Ho == dy8.size(1) && s.Wo == dy8.size(2) && K == dy8.size(3) && s.N == dy8.size(0),
              "conv_wgrad_fp8: dy shape mismatch");
  const Tensor* o = opt(out);
  if (o) check_krsc_out(*o, K, C, R, S);
  c10::hip::HIPGuard g(x8.get_device());
  SideStream ss(side, (c10::DeviceIndex)x8.get_device());
  Tensor dwp = o ? *o : at::empty({K, R, S, C}, x8.options().dtype(at::kFloat));
  pdt::launch_conv_wgrad_fp8(dy8.data_ptr<uint8_t>(), x8.data_ptr<uint8_t>(), dyq, xq, dwp.data_ptr<float>(), s,
                             o != nullptr, ss.stream());
  // a consumed BN-sum accumulator: cleared by a memset AFTER the kernel (the bf16 weight gradient
  // clears it in its workgroup 0 instead; done that way here, the fp8 ResNet-50 parity runs fell
  // behind in 4 of 7 runs against 0 of 7 with the memset -- profiles/r6_fp8_parity.txt)
  if (const Tensor* z = opt(zero))
    TORCH_CHECK(hipMemsetAsync(z->data_ptr(), 0, z->nbytes(), ss.stream()) == hipSuccess, "memset");
  ss.keep({&dy8, &x8, &dy_deq, &x_deq});
  return o ? dwp : dwp.permute({0, 3, 1, 2});
}

py::dict plan_dict(std::initializer_list<const char*> keys, const int* v) {
  py::dict d;
  for (const char* k : keys) d[k] = *v++;
  return d;
}

pdt::ConvShape plan_shape(const std::vector<int64_t>& xs, const std::vector<int64_t>& ws, int stride, int pad) {
  TORCH_CHECK(xs.size() == 4 && ws.size() == 4, "x_shape [N,H,W,C], w_shape [K,C,R,S]");
  return shape_of((int)xs[0], (int)xs[1], (int)xs[2], (int)xs[3], (int)ws[0], (int)ws[2], (int)ws[3], stride, pad);
}

// -------------------------------------------------------------------- stem
// the super-pixel conv shape of the stem: image [N,Hp,Wsp,8], weights [K,R,Sp,8], stride (2, 1)
pdt::ConvShape stem_shape(int N, int Hp, int Wsp, int K, int R, int Sp, int Ho, int Wo) {
  pdt::ConvShape s;
  s.N = N; s.H = Hp; s.W = Wsp; s.C = 8; s.K = K; s.R = R; s.S = Sp;
  s.Ho = Ho; s.Wo = Wo; s.stride = 2; s.stride_w = 1; s.pad = 0;
  return s;
}

// 7x7/s2 stem with C <= 4 input channels as a super-pixel conv (kernels.h): returns
// (xsp, y, part, grows) -- xsp is the bf16 super-pixel image (kept for the weight gradient)
std::tuple<Tensor, Tensor, Tensor, int64_t> stem_conv_fwd(const Tensor& x, const Tensor& w, int64_t stride,
                                                          int64_t pad, bool stats) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat && x.dim() == 4, "stem: image must be fp32 NCHW");
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == at::kFloat && w.dim() == 4, "stem: weight must be fp32 4-D");
  TORCH_CHECK(stride == 2 && x.size(1) <= 4 && w.size(1) == x.size(1), "stem: stride 2, <= 4 channels");
  c10::hip::HIPGuard g(x.get_device());
  Tensor xc = x.contiguous();
  const int N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const int K = w.size(0), R = w.size(2), S = w.size(3);
  const int Ho = (H + 2 * pad - R) / 2 + 1, Wo = (W + 2 * pad - S) / 2 + 1;
  const int Sp = (S + 2) / 2, Hp = H + 2 * pad, Wsp = Wo + Sp - 1;
  TORCH_CHECK(2 * (Ho - 1) + R <= Hp, "stem: padded height too small");
  auto xsp = at::empty({N, Hp, Wsp, 8}, x.options().dtype(at::kBFloat16));
  hipStream_t st = cur_stream(x);
  pdt::launch_stem_image(xc.data_ptr<float>(), bf(xsp), N, C, H, W, (int)pad, Hp, Wsp, st);
  auto wsp = at::empty({K, R, Sp, 8}, w.options().dtype(at::kBFloat16));
  int64_t ws[4] = {w.stride(0), w.stride(1), w.stride(2), w.stride(3)};
  pdt::launch_stem_pack_weight(w.data_ptr<float>(), ws, bf(wsp), K, C, R, S, Sp, st);
  auto s = stem_shape(N, Hp, Wsp, K, R, Sp, Ho, Wo);
  TORCH_CHECK(xsp.numel() < (int64_t(1) << 30), "stem: image too large for 32-bit addressing");
  auto y = at::empty({N, Ho, Wo, K}, xsp.options());
  Tensor part;
  float* pp = nullptr;
  const int M = N * Ho * Wo;
  const bool halo = pdt::stem_halo_supported(K, R, Sp, Wo);
  // BN partial groups: one per output row on the halo kernel, one per NT row tile otherwise
  const int grows = halo ? Wo : pdt::conv_nt_group_rows(M, K, R * Sp * 8 * 2);
  if (stats) {
    part = at::empty({(M + grows - 1) / grows, 2, K}, x.options());
    pp = part.data_ptr<float>();
  }
  if (halo) pdt::launch_stem_conv_fwd(cbf(xsp), cbf(wsp), bf(y), pp, N, Hp, Wsp, Ho, Wo, st);
  else pdt::launch_conv_fwd(cbf(xsp), cbf(wsp), bf(y), pp, s, st);
  return {xsp, y, part, (int64_t)grows};
}

// weight gradient of the stem from the super-pixel image; accumulates into `out` (fp32 [K,C,R,S],
// any strides) when given, else returns a fresh channels_last tensor
Tensor stem_wgrad(const Tensor& dy, const Tensor& xsp, std::vector<int64_t> wsz, bool deterministic,
                  const std::optional<Tensor>& out) {
  check_bf16_nhwc(dy, "dy");
  check_bf16_nhwc(xsp, "xsp");
  TORCH_CHECK(wsz.size() == 4, "weight shape must be [K,C,R,S]");
  c10::hip::HIPGuard g(dy.get_device());
  const int K = wsz[0], C = wsz[1], R = wsz[2], S = wsz[3];
  const int Sp = (S + 2) / 2;
  auto s = stem_shape(xsp.size(0), xsp.size(1), xsp.size(2), K, R, Sp, dy.size(1), dy.size(2));
  TORCH_CHECK(dy.size(3) == K && s.Wo + Sp - 1 == s.W, "stem_wgrad: shape mismatch");
  auto fopt = dy.options().dtype(at::kFloat);
  size_t wsn = pdt::conv_wgrad_ws_floats(s, deterministic);
  Tensor wsb = wsn ? at::empty({(int64_t)wsn}, fopt) : Tensor();
  auto dwsp = at::empty({K, R, Sp, 8}, fopt);
  hipStream_t st = cur_stream(dy);
  pdt::launch_conv_wgrad(cbf(dy), cbf(xsp), dwsp.data_ptr<float>(), wsn ? wsb.data_ptr<float>() : nullptr,
                         s, deterministic, false, st);
  return stem_unpack(dwsp, out, K, C, R, S, Sp, st);
}

// stem backward with the BN/pool apply fused into the weight gradient: accumulates dW into `out`
// (fp32 [K,C,R,S], any strides) when given, else returns a fresh channels_last tensor
Tensor stem_bwd_fused(const Tensor& dpool, const Tensor& idx, const Tensor& y, const Tensor& stats,
                      const Tensor& gamma, const Tensor& sums, bool training, const Tensor& xsp,
                      std::vector<int64_t> wsz, bool deterministic, const std::optional<Tensor>& out) {
  check_bf16_nhwc(dpool, "dpool");
  check_bf16_nhwc(y, "y");
  check_bf16_nhwc(xsp, "xsp");
  TORCH_CHECK(wsz.size() == 4, "weight shape must be [K,C,R,S]");
  TORCH_CHECK(idx.is_cuda() && idx.scalar_type() == at::kByte && idx.is_contiguous() &&
              idx.numel() == dpool.numel(), "idx: uint8 argmax map like dpool");
  TORCH_CHECK(stats.scalar_type() == at::kFloat && stats.numel() == 4 * y.size(3) &&
              sums.scalar_type() == at::kFloat && sums.numel() == 2 * y.size(3), "stats [4][K], sums [2][K]");
  c10::hip::HIPGuard g(y.get_device());
  const int K = wsz[0], C = wsz[1], R = wsz[2], S = wsz[3];
  const int Sp = (S + 2) / 2;
  const int N = y.size(0), Ho = y.size(1), Wo = y.size(2);
  TORCH_CHECK(y.size(3) == K && pdt::stem_bwd_fused_supported(K, R, Sp, Ho, Wo), "stem_bwd_fused: unsupported shape");
  TORCH_CHECK(dpool.size(0) == N && dpool.size(1) == Ho / 2 && dpool.size(2) == Wo / 2 && dpool.size(3) == K,
              "stem_bwd_fused: dpool must be the 3x3/s2/p1 max pool of y");
  TORCH_CHECK(xsp.size(0) == N && xsp.size(2) == Wo + Sp - 1 && xsp.size(3) == 8, "stem_bwd_fused: xsp shape");
  auto fopt = y.options().dtype(at::kFloat);
  auto dwsp = at::empty({K, R, Sp, 8}, fopt);
  Tensor wsb;
  if (deterministic) wsb = at::empty({(int64_t)pdt::stem_bwd_fused_blocks(N, Ho) * K * R * Sp * 8}, fopt);
  hipStream_t st = cur_stream(y);
  pdt::launch_stem_bwd_fused(cbf(dpool), idx.data_ptr<uint8_t>(), cbf(y), stats.data_ptr<float>(),
                             gamma.data_ptr<float>(), sums.data_ptr<float>(), training, cbf(xsp), N, Ho, Wo,
                             xsp.size(1), xsp.size(2), dwsp.data_ptr<float>(),
                             deterministic ? wsb.data_ptr<float>() : nullptr, st);
  return stem_unpack(dwsp, out, K, C, R, S, Sp, st);
}

// a, b: uint8 [64, 32] per-lane operand registers; returns fp32 [64, 4] accumulators
Tensor mfma_f8_probe(const Tensor& a, const Tensor& b, int64_t fmt_a, int64_t fmt_b, int64_t scale_a,
                     int64_t scale_b, bool use_scale) {
  check_cuda(a, "a");
  check_cuda(b, "b");
  TORCH_CHECK(a.scalar_type() == at::kByte && b.scalar_type() == at::kByte && a.numel() == 64 * 32 &&
              b.numel() == 64 * 32, "probe operands: uint8 [64, 32]");
  TORCH_CHECK((fmt_a == 0 || fmt_a == 1) && (fmt_b == 0 || fmt_b == 1), "fmt: 0 = e4m3, 1 = e5m2");
  c10::hip::HIPGuard g(a.get_device());
  auto d = at::empty({64, 4}, a.options().dtype(at::kFloat));
  pdt::launch_mfma_f8_probe(a.data_ptr(), b.data_ptr(), d.data_ptr<float>(), (int)fmt_a, (int)fmt_b,
                            (int)scale_a, (int)scale_b, use_scale ? 1 : 0, cur_stream(a));
  return d;
}

}  // namespace

void register_conv(py::module_& m) {
  def_op(m, "image_to_nhwc", &image_to_nhwc);
  def_op(m, "pack_weight", &pack_weight, py::arg("w"), py::arg("cpad") = 0);
  def_op(m, "pack_weight_t", &pack_weight_t);
  def_op(m, "pack_weight_fp8", &pack_weight_fp8, py::arg("w"), py::arg("cpad") = 0, py::arg("act_deq") = py::none());
  def_op(m, "cast_to_bf16", &cast_to_bf16);
  def_op(m, "pack_t_batched", &pack_t_batched);
  m.def("pack_t_entry_bytes", &pack_t_entry_bytes);
  def_op(m, "conv_fwd", &conv_fwd, py::arg("x"), py::arg("wk"), py::arg("stride"), py::arg("pad"), py::arg("stats"));
  def_op(m, "conv_fwd_bn", &conv_fwd_bn, py::arg("x"), py::arg("wk"), py::arg("stride"), py::arg("pad"),
         py::arg("count"), py::arg("rm"), py::arg("rv"), py::arg("gamma"), py::arg("beta"), py::arg("momentum"),
         py::arg("eps"), py::arg("acc") = py::none());
  def_op(m, "conv_fwd_fp8", &conv_fwd_fp8, py::arg("x"), py::arg("wq"), py::arg("oscale"), py::arg("stride"),
         py::arg("pad"), py::arg("stats"), py::arg("ascale") = py::none(), py::arg("bn") = py::none());
  def_op(m, "conv_dgrad", &conv_dgrad, py::arg("dy"), py::arg("w"), py::arg("x_shape"), py::arg("stride"),
         py::arg("pad"), py::arg("addend") = py::none(), py::arg("wt") = py::none());
  def_op(m, "conv_dgrad_bn", &conv_dgrad_bn, py::arg("dy"), py::arg("w"), py::arg("x_shape"), py::arg("stride"),
         py::arg("pad"), py::arg("addend"), py::arg("y"), py::arg("z"), py::arg("stats"), py::arg("mask"),
         py::arg("dgamma") = py::none(), py::arg("dbeta") = py::none(), py::arg("wt") = py::none(),
         py::arg("acc") = py::none(), py::arg("y2") = py::none(), py::arg("stats2") = py::none(),
         py::arg("acc2") = py::none());
  def_op(m, "conv_dgrad_bn_fold", &conv_dgrad_bn_fold, py::arg("g"), py::arg("z_in"), py::arg("wfold"),
         py::arg("bias"), py::arg("y"), py::arg("z"), py::arg("stats"), py::arg("mask"), py::arg("acc") = py::none(),
         py::arg("dgamma") = py::none(), py::arg("dbeta") = py::none());
  def_op(m, "conv_dgrad_fp8", &conv_dgrad_fp8, py::arg("dy8"), py::arg("wt8"), py::arg("wscale"), py::arg("ascale"),
         py::arg("x_shape"), py::arg("stride"), py::arg("pad"), py::arg("addend") = py::none());
  def_op(m, "conv_dgrad_bn_fp8", &conv_dgrad_bn_fp8, py::arg("dy8"), py::arg("wt8"), py::arg("wscale"),
         py::arg("ascale"), py::arg("x_shape"), py::arg("stride"), py::arg("pad"), py::arg("addend"), py::arg("y"),
         py::arg("z"), py::arg("stats"), py::arg("mask"), py::arg("dgamma") = py::none(),
         py::arg("dbeta") = py::none(), py::arg("acc") = py::none());
  def_op(m, "conv_wgrad", &conv_wgrad, py::arg("dy"), py::arg("x"), py::arg("w_shape"), py::arg("stride"),
         py::arg("pad"), py::arg("deterministic") = false, py::arg("out") = py::none());
  def_op(m, "conv_wgrad_side", &conv_wgrad_side, py::arg("side"), py::arg("dy"), py::arg("x"), py::arg("w_shape"),
         py::arg("stride"), py::arg("pad"), py::arg("deterministic") = false, py::arg("out") = py::none(),
         py::arg("zero") = py::none());
  def_op(m, "conv_wgrad_fp8", &conv_wgrad_fp8, py::arg("side"), py::arg("dy8"), py::arg("x8"), py::arg("dy_deq"),
         py::arg("x_deq"), py::arg("w_shape"), py::arg("stride"), py::arg("pad"), py::arg("out") = py::none(),
         py::arg("zero") = py::none());
  m.def("conv_wgrad_fp8_plan", [](std::vector<int64_t> x_shape, std::vector<int64_t> w_shape, int stride, int pad) {
    int o[4];
    pdt::conv_wgrad_fp8_plan(plan_shape(x_shape, w_shape, stride, pad), o);
    return plan_dict({"bm", "tiles", "splits", "steps_per_split"}, o);
  }, py::arg("x_shape"), py::arg("w_shape"), py::arg("stride"), py::arg("pad"));
  m.def("conv_wgrad_plan", [](std::vector<int64_t> x_shape, std::vector<int64_t> w_shape, int stride, int pad,
                              bool deterministic) {
    int o[4];
    pdt::conv_wgrad_plan(plan_shape(x_shape, w_shape, stride, pad), deterministic, o);
    return plan_dict({"bm", "bn", "tiles", "splits"}, o);
  }, py::arg("x_shape"), py::arg("w_shape"), py::arg("stride"), py::arg("pad"), py::arg("deterministic") = false);
  m.def("conv_wgrad_set_cu_reserve", &pdt::conv_wgrad_set_cu_reserve, py::arg("n"),
        "CUs the weight-gradient split-K plan leaves to the gradient-collective kernels");
  m.def("conv_wgrad_cu_reserve", &pdt::conv_wgrad_cu_reserve);
  m.def("conv_nt_group_rows", &pdt::conv_nt_group_rows, py::arg("M"), py::arg("Nout"), py::arg("kg_bytes"));
  m.def("conv_nt_force", &pdt::conv_nt_force, py::arg("k32") = -1, py::arg("mid") = -1, py::arg("wide") = -1);
  m.def("conv_nt_tile", [](int M, int Nout, int kg_bytes) {
    int bm = 0, bn = 0;
    pdt::conv_nt_tile(M, Nout, kg_bytes, &bm, &bn);
    return py::make_tuple(bm, bn);
  }, py::arg("M"), py::arg("Nout"), py::arg("kg_bytes"));
  m.def("nt_timing_fetch", [](int n) {
    // PDT_NT_TIMING variant builds: [n] per-block phase timestamps of NT launches (else empty)
    auto out = torch::zeros({n}, torch::dtype(torch::kInt64));
    const int got = pdt::nt_timing_fetch(reinterpret_cast<unsigned long long*>(out.data_ptr<int64_t>()), n);
    return out.narrow(0, 0, got);
  }, py::arg("n"));
  def_op(m, "stem_conv_fwd", &stem_conv_fwd, py::arg("x"), py::arg("w"), py::arg("stride"), py::arg("pad"),
         py::arg("stats"));
  def_op(m, "stem_wgrad", &stem_wgrad, py::arg("dy"), py::arg("xsp"), py::arg("w_shape"),
         py::arg("deterministic") = false, py::arg("out") = py::none());
  def_op(m, "stem_bwd_fused", &stem_bwd_fused, py::arg("dpool"), py::arg("idx"), py::arg("y"), py::arg("stats"),
         py::arg("gamma"), py::arg("sums"), py::arg("training"), py::arg("xsp"), py::arg("w_shape"),
         py::arg("deterministic") = false, py::arg("out") = py::none());
  m.def("stem_bwd_fused_supported", &pdt::stem_bwd_fused_supported, py::arg("K"), py::arg("R"), py::arg("Sp"),
        py::arg("Ho"), py::arg("Wo"));
  def_op(m, "mfma_f8_probe", &mfma_f8_probe, py::arg("a"), py::arg("b"), py::arg("fmt_a") = 0, py::arg("fmt_b") = 0,
         py::arg("scale_a") = 127, py::arg("scale_b") = 127, py::arg("use_scale") = true);
}
