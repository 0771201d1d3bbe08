// Bindings of the BatchNorm kernels (finalize, apply, backward, the folded backward), the pooling
// kernels and the fp8 quantisation.
#include "bind_util.h"

using namespace pdt::bind;

Tensor pdt::bind::bn_finalize(const Tensor& part, int64_t count, const Tensor& rm, const Tensor& rv,
                              const Tensor& gamma, const Tensor& beta, double momentum, double eps,
                              int64_t grows_in) {
  check_cuda(part, "part");
  c10::hip::HIPGuard g(part.get_device());
  int ng = part.size(0), K = part.size(2);
  // the producing conv's row group is its NT tile's BM (64, 128 or 256; conv_nt_group_rows): the
  // only one of those giving ng groups over `count` rows; a single group covers every row.  A
  // producer with another grouping (the halo stem: one group per output row) passes grows_in.
  int grows = 0;
  if (grows_in > 0) {
    TORCH_CHECK((count + grows_in - 1) / grows_in == ng, "bn_finalize: grows does not match the partials");
    grows = (int)grows_in;
  } else if (ng == 1) {
    grows = (int)count;
  } else {
    for (int g : {64, 128, 256})
      if ((count + g - 1) / g == ng) { grows = g; break; }
  }
  TORCH_CHECK(grows > 0, "bn_finalize: partial layout mismatch");
  int P = pdt::bn_finalize_partitions(ng);
  auto out = at::empty({4 * K + 3 * K * P}, part.options());
  TORCH_CHECK(gamma.scalar_type() == at::kFloat && rm.scalar_type() == at::kFloat, "BN params must be fp32");
  pdt::launch_bn_finalize(part.data_ptr<float>(), ng, grows, (int)count, K,
                          rm.defined() ? rm.data_ptr<float>() : nullptr,
                          rv.defined() ? rv.data_ptr<float>() : nullptr, gamma.data_ptr<float>(),
                          beta.data_ptr<float>(), (float)momentum, (float)eps,
                          out.data_ptr<float>(), cur_stream(part));
  return out.narrow(0, 0, 4 * K).view({4, K});
}

namespace {

Tensor bn_eval_params(const Tensor& rm, const Tensor& rv, const Tensor& gamma, const Tensor& beta,
                      double eps) {
  check_cuda(rm, "running_mean");
  c10::hip::HIPGuard g(rm.get_device());
  int K = rm.numel();
  auto out = at::empty({4, K}, rm.options().dtype(at::kFloat));
  pdt::launch_bn_eval_params(rm.data_ptr<float>(), rv.data_ptr<float>(), gamma.data_ptr<float>(),
                             beta.data_ptr<float>(), (float)eps, K, out.data_ptr<float>(),
                             cur_stream(rm));
  return out;
}

// optional BatchNorm of the residual (res_scale / res_shift: fp32 [K]); returns their pointers
std::pair<const float*, const float*> res_bn_args(const std::optional<Tensor>& res,
                                                  const std::optional<Tensor>& rsc,
                                                  const std::optional<Tensor>& rsh, int64_t K) {
  const Tensor* sc = opt(rsc);
  const Tensor* sh = opt(rsh);
  TORCH_CHECK(!sc == !sh, "res_scale and res_shift go together");
  if (!sc) return {nullptr, nullptr};
  TORCH_CHECK(opt(res), "a residual BatchNorm needs the residual");
  for (const Tensor* t : {sc, sh})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kFloat && t->is_contiguous() && t->numel() == K,
                "res_scale / res_shift must be contiguous fp32 [K] device tensors");
  return {sc->data_ptr<float>(), sh->data_ptr<float>()};
}

Tensor bn_act_fwd(const Tensor& y, const Tensor& scale, const Tensor& shift,
                  const std::optional<Tensor>& res, bool relu, const std::optional<Tensor>& rsc,
                  const std::optional<Tensor>& rsh, const std::optional<Tensor>& csum) {
  check_bf16_nhwc(y, "y");
  c10::hip::HIPGuard g(y.get_device());
  int K = y.size(3);
  int64_t M = y.numel() / K;
  const uint16_t* rp = residual_ptr(res, y);
  auto rbn = res_bn_args(res, rsc, rsh, K);
  float* cs = nullptr;
  if (const Tensor* c = opt(csum)) {  // per-channel sums of z into fp32 [S, K] slots (atomic)
    check_cuda(*c, "csum");
    TORCH_CHECK(c->scalar_type() == at::kFloat && c->numel() == (int64_t)pdt::bn_csum_slots() * K,
                "csum must be a contiguous fp32 [bn_csum_slots(), K] device tensor");
    cs = c->data_ptr<float>();
  }
  auto z = at::empty_like(y);
  pdt::launch_bn_act_fwd(cbf(y), scale.data_ptr<float>(), shift.data_ptr<float>(), rp, relu, bf(z), M,
                         K, cur_stream(y), nullptr, rbn.first, rbn.second, cs);
  return z;
}

// (z, zmask): bn_act_fwd with ReLU that also writes the 1-bit-per-element ReLU mask (uint8, one
// byte per 8 channels) for a later BN-fused dgrad (mask mode 3)
std::tuple<Tensor, Tensor> bn_act_fwd_mask(const Tensor& y, const Tensor& scale, const Tensor& shift,
                                           const std::optional<Tensor>& res,
                                           const std::optional<Tensor>& rsc,
                                           const std::optional<Tensor>& rsh) {
  check_bf16_nhwc(y, "y");
  c10::hip::HIPGuard g(y.get_device());
  int K = y.size(3);
  int64_t M = y.numel() / K;
  const uint16_t* rp = residual_ptr(res, y);
  auto rbn = res_bn_args(res, rsc, rsh, K);
  auto z = at::empty_like(y);
  auto zm = at::empty({y.numel() / 8}, y.options().dtype(at::kByte));
  pdt::launch_bn_act_fwd(cbf(y), scale.data_ptr<float>(), shift.data_ptr<float>(), rp, true, bf(z), M, K,
                         cur_stream(y), zm.data_ptr<uint8_t>(), rbn.first, rbn.second);
  return {z, zm};
}

// (z, q, zmask); zmask is undefined unless want_mask (needs relu)
std::tuple<Tensor, Tensor, Tensor> bn_act_fwd_q8(const Tensor& y, const Tensor& scale, const Tensor& shift,
                                                 const std::optional<Tensor>& res, bool relu, Tensor state,
                                                 int64_t slot, bool want_mask, bool want_z) {
  check_bf16_nhwc(y, "y");
  check_state(state, slot);
  c10::hip::HIPGuard g(y.get_device());
  int K = y.size(3);
  int64_t M = y.numel() / K;
  const uint16_t* rp = residual_ptr(res, y);
  TORCH_CHECK(!want_mask || relu, "a ReLU mask needs relu");
  Tensor z;
  if (want_z) z = at::empty_like(y);  // else: fp8-only activation, every consumer reads q
  auto q = at::empty(y.sizes(), y.options().dtype(at::kByte));
  Tensor zm;
  if (want_mask) zm = at::empty({y.numel() / 8}, y.options().dtype(at::kByte));
  pdt::launch_bn_act_fwd_q8(cbf(y), scale.data_ptr<float>(), shift.data_ptr<float>(), rp, relu,
                            want_z ? bf(z) : nullptr,
                            q.data_ptr<uint8_t>(), M, K, state.data_ptr<float>(), (int)slot, cur_stream(y),
                            want_mask ? zm.data_ptr<uint8_t>() : nullptr);
  return {z, q, zm};
}

// ---------------------------------------------------------------- backward
Tensor bn_act_bwd_reduce(const Tensor& dz, const Tensor& z, const Tensor& y, const Tensor& stats,
                         int64_t mask, const std::optional<Tensor>& dgamma,
                         const std::optional<Tensor>& dbeta) {
  auto b = bn_bwd_prologue(dz, y, stats, mask, z);
  auto pg = bn_param_sinks(dgamma, dbeta, b.K);
  c10::hip::HIPGuard g(dz.get_device());
  auto fopt = y.options().dtype(at::kFloat);
  auto ws = at::empty({(int64_t)pdt::bn_bwd_ws_floats(b.M, b.K)}, fopt);
  auto sums = at::empty({2, b.K}, fopt);
  pdt::launch_bn_act_bwd_reduce(cbf(dz), b.z, cbf(y), stats.data_ptr<float>(), (int)mask, b.M, b.K,
                                ws.data_ptr<float>(), sums.data_ptr<float>(), pg.first, pg.second,
                                cur_stream(y));
  return sums;
}

std::tuple<Tensor, Tensor> bn_act_bwd_apply(const Tensor& dz, const Tensor& z, const Tensor& y,
                                            const Tensor& stats, const Tensor& gamma,
                                            const Tensor& sums, int64_t mask, bool training,
                                            bool want_dres, const std::optional<Tensor>& dgamma,
                                            const std::optional<Tensor>& dbeta) {
  auto b = bn_bwd_prologue(dz, y, stats, mask, z, /*pow2_groups=*/false);
  auto pg = bn_param_sinks(dgamma, dbeta, b.K);
  c10::hip::HIPGuard g(dz.get_device());
  auto dy = at::empty_like(dz);
  Tensor dres;
  if (want_dres) dres = at::empty_like(dz);
  pdt::launch_bn_act_bwd_apply(cbf(dz), b.z, cbf(y), stats.data_ptr<float>(), gamma.data_ptr<float>(),
                               sums.data_ptr<float>(), (int)mask, training, b.M, b.K, bf(dy),
                               want_dres ? bf(dres) : nullptr, cur_stream(dz), pg.first, pg.second);
  return {dy, dres};
}

// (dy, dres, dy8): bn_act_bwd_apply (training) that also emits dy8 = e5m2(dy * s_t)
std::tuple<Tensor, Tensor, Tensor> bn_act_bwd_apply_q8(const Tensor& dz, const Tensor& z, const Tensor& y,
                                                       const Tensor& stats, const Tensor& gamma,
                                                       const Tensor& sums, int64_t mask, bool want_dres,
                                                       Tensor state, int64_t slot, bool want_dy,
                                                       const std::optional<Tensor>& dgamma,
                                                       const std::optional<Tensor>& dbeta) {
  auto b = bn_bwd_prologue(dz, y, stats, mask, z);
  check_state(state, slot);
  auto pg = bn_param_sinks(dgamma, dbeta, b.K);
  c10::hip::HIPGuard g(dz.get_device());
  Tensor dy, dres;
  if (want_dy) dy = at::empty_like(dz);  // else: fp8-only dy, every consumer reads dy8
  if (want_dres) dres = at::empty_like(dz);
  auto dy8 = at::empty(dz.sizes(), dz.options().dtype(at::kByte));
  pdt::launch_bn_act_bwd_apply_q8(cbf(dz), b.z, cbf(y), stats.data_ptr<float>(), gamma.data_ptr<float>(),
                                  sums.data_ptr<float>(), (int)mask, true, b.M, b.K, want_dy ? bf(dy) : nullptr,
                                  want_dres ? bf(dres) : nullptr, dy8.data_ptr<uint8_t>(),
                                  state.data_ptr<float>(), (int)slot, cur_stream(dz), pg.first, pg.second);
  return {dy, dres, dy8};
}

// ------------------------------------------------------- folded BN backward
void check_fold_wt(const Tensor& wt) {
  check_cuda(wt, "wt");
  TORCH_CHECK(wt.scalar_type() == at::kBFloat16 && wt.numel() == wt.size(0) * wt.size(-1),
              "wt must be contiguous bf16 [C][K]");
}

// Folded BN backward (kernels.h DgradFold): (wfold [C][K + C] bf16, bias [C] fp32) for the 1x1 conv
// whose transposed bf16 weights are wt [C][K] (or [C][1][1][K]), from its output BN's statistics,
// gamma and backward sums over `count` rows.
std::tuple<Tensor, Tensor> bn_fold_weights(const Tensor& wt, const Tensor& stats, const Tensor& gamma,
                                           const Tensor& sums, int64_t count) {
  check_fold_wt(wt);
  const int C = wt.size(0), K = wt.size(-1);
  check_stats(stats, K);
  TORCH_CHECK(gamma.scalar_type() == at::kFloat && gamma.numel() == K, "gamma: fp32 [K]");
  TORCH_CHECK(sums.scalar_type() == at::kFloat && sums.is_contiguous() && sums.numel() == 2 * K, "sums: fp32 [2, K]");
  c10::hip::HIPGuard g(wt.get_device());
  auto wfold = at::empty({C, K + C}, wt.options());
  auto bias_ws = at::empty({pdt::bn_fold_weights_ws_floats(C, K)}, stats.options());  // bias, then the kernel's scratch
  auto bias = bias_ws.narrow(0, 0, C);
  pdt::launch_bn_fold_weights(cbf(wt), stats.data_ptr<float>(), gamma.data_ptr<float>(), sums.data_ptr<float>(),
                              (int)count, C, K, bf(wfold), bias.data_ptr<float>(), cur_stream(wt));
  return {wfold, bias};
}

// Weight gradient of a folded unit (kernels.h launch_bn_fold_wgrad): out [K,C,1,1] fp32 (a KRSC-dense
// view, e.g. the flat gradient buffer) += diag(k1) t1 + diag(a) W gram + b colsum^T with W the bf16
// mirror wt [C][K] (the operand bn_fold_weights read); dgamma/dbeta (optional) take the BN parameter
// gradients.  done (an int32 [1] counter, 0 between calls): consume mode -- t1 and gram are persistent
// workspaces the kernel clears after reading, and `sums` too when zero_sums.
void bn_fold_wgrad(Tensor t1, Tensor gram, const Tensor& colsum, const Tensor& wt,
                   const Tensor& stats, const Tensor& gamma, const Tensor& sums, int64_t count, Tensor out,
                   const std::optional<Tensor>& dgamma, const std::optional<Tensor>& dbeta,
                   const std::optional<Tensor>& done, bool zero_sums) {
  check_fold_wt(wt);
  check_cuda(colsum, "colsum");
  const int C = wt.size(0), K = wt.size(-1);
  TORCH_CHECK(t1.scalar_type() == at::kFloat && t1.numel() == (int64_t)K * C, "t1: fp32 [K, C]");
  TORCH_CHECK(gram.scalar_type() == at::kFloat && gram.numel() == (int64_t)C * C, "gram: fp32 [C, C]");
  // colsum: fp32 [C] (a reduction pass) or [S, C] (bn_act_fwd's S = bn_csum_slots() slots, consume
  // mode: re-zeroed)
  const int S = pdt::bn_csum_slots();
  TORCH_CHECK(colsum.scalar_type() == at::kFloat &&
              (colsum.numel() == C || (colsum.dim() == 2 && colsum.size(0) == S && colsum.size(1) == C)),
              "colsum: fp32 [C] or [bn_csum_slots(), C]");
  const int csum_slots = colsum.dim() == 2 ? S : 1;
  TORCH_CHECK(out.scalar_type() == at::kFloat && out.numel() == (int64_t)K * C, "out: fp32 [K, C, 1, 1]");
  for (const Tensor* x : {(const Tensor*)&t1, (const Tensor*)&gram, (const Tensor*)&out}) {
    // 1x1: [K,C,1,1] in either memory format is [K][C] memory when its two big strides are (C, 1)
    TORCH_CHECK(x->stride(0) == x->size(1) && x->stride(1) == 1, "fold wgrad: [K][C]-dense operands");
  }
  TORCH_CHECK(stats.numel() == 4 * K && gamma.numel() == K && sums.numel() == 2 * K && sums.is_contiguous(),
              "BN operands: [4,K], [K], [2,K]");
  int* dp = nullptr;
  if (const Tensor* d = opt(done)) {
    TORCH_CHECK(d->is_cuda() && d->scalar_type() == at::kInt && d->numel() >= C / 64 + 1,
                "done: int32 device counters [C / 64 + 1]");
    dp = d->data_ptr<int>();
  }
  TORCH_CHECK(!zero_sums || dp != nullptr, "zero_sums needs the completion counter");
  c10::hip::HIPGuard g(wt.get_device());
  auto pg = bn_param_sinks(dgamma, dbeta, K);
  pdt::launch_bn_fold_wgrad(t1.data_ptr<float>(), gram.data_ptr<float>(), colsum.data_ptr<float>(), cbf(wt),
                            stats.data_ptr<float>(), gamma.data_ptr<float>(), sums.data_ptr<float>(), (int)count,
                            C, K, out.data_ptr<float>(), pg.first, pg.second, dp, zero_sums, cur_stream(wt),
                            csum_slots);
}

// -------------------------------------------------------------------- pool
std::tuple<Tensor, Tensor> maxpool_fwd(const Tensor& x) {
  check_bf16_nhwc(x, "x");
  c10::hip::HIPGuard g(x.get_device());
  int N = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
  auto y = at::empty({N, Ho, Wo, C}, x.options());
  auto idx = at::empty({N, Ho, Wo, C}, x.options().dtype(at::kByte));
  pdt::launch_maxpool_fwd(cbf(x), bf(y), idx.data_ptr<uint8_t>(), N, H, W, C, Ho, Wo, cur_stream(x));
  return {y, idx};
}

Tensor maxpool_bwd(const Tensor& dy, const Tensor& idx, int64_t H, int64_t W) {
  check_bf16_nhwc(dy, "dy");
  c10::hip::HIPGuard g(dy.get_device());
  int N = dy.size(0), Ho = dy.size(1), Wo = dy.size(2), C = dy.size(3);
  auto dx = at::empty({N, H, W, C}, dy.options());
  pdt::launch_maxpool_bwd(cbf(dy), idx.data_ptr<uint8_t>(), bf(dx), N, H, W, C, Ho, Wo, cur_stream(dy));
  return dx;
}

// stem: (pooled, idx) = maxpool3x3s2(relu(y*scale + shift)) without writing the ReLU output;
// with argmax_y also u = y at each window's argmax (what the BN backward reduction needs from y:
// it then streams the pooled tensors instead of gathering over the full-resolution y)
py::tuple bn_relu_maxpool(const Tensor& y, const Tensor& scale, const Tensor& shift, bool argmax_y) {
  check_bf16_nhwc(y, "y");
  check_cuda(scale, "scale");
  check_cuda(shift, "shift");
  c10::hip::HIPGuard g(y.get_device());
  int N = y.size(0), H = y.size(1), W = y.size(2), C = y.size(3);
  TORCH_CHECK(scale.numel() == C && shift.numel() == C && scale.scalar_type() == at::kFloat &&
              shift.scalar_type() == at::kFloat, "scale/shift must be fp32 [C]");
  int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
  auto out = at::empty({N, Ho, Wo, C}, y.options());
  auto idx = at::empty({N, Ho, Wo, C}, y.options().dtype(at::kByte));
  Tensor u;
  if (argmax_y) u = at::empty({N, Ho, Wo, C}, y.options());
  pdt::launch_bn_relu_maxpool(cbf(y), scale.data_ptr<float>(), shift.data_ptr<float>(), bf(out),
                              idx.data_ptr<uint8_t>(), argmax_y ? bf(u) : nullptr, N, H, W, C, Ho, Wo,
                              cur_stream(y));
  if (argmax_y) return py::make_tuple(out, idx, u);
  return py::make_tuple(out, idx);
}

// gradient of the stem's fused BN/ReLU/max pool over y with statistics [4, K]
void check_pool_grad(const Tensor& dpool, const Tensor& idx, const Tensor& y, const Tensor& stats) {
  check_bf16_nhwc(dpool, "dpool");
  check_bf16_nhwc(y, "y");
  check_cuda(idx, "idx");
  TORCH_CHECK(idx.scalar_type() == at::kByte && idx.sizes() == dpool.sizes(), "idx must be uint8 like dpool");
  TORCH_CHECK(dpool.size(0) == y.size(0) && dpool.size(3) == y.size(3) &&
              dpool.size(1) == (y.size(1) - 1) / 2 + 1 && dpool.size(2) == (y.size(2) - 1) / 2 + 1,
              "dpool must be the 3x3/s2/p1 max pool of y");
  check_stats(stats, y.size(3));
}

// sums[2][K] of the stem BN backward with dz = maxpool_bwd(dpool, idx) gathered on the fly
Tensor pool_bn_bwd_reduce(const Tensor& dpool, const Tensor& idx, const Tensor& y, const Tensor& stats,
                          const std::optional<Tensor>& dgamma, const std::optional<Tensor>& dbeta) {
  check_pool_grad(dpool, idx, y, stats);
  int N = y.size(0), H = y.size(1), W = y.size(2), K = y.size(3);
  auto pg = bn_param_sinks(dgamma, dbeta, K);
  c10::hip::HIPGuard g(y.get_device());
  auto fopt = y.options().dtype(at::kFloat);
  auto ws = at::empty({(int64_t)pdt::pool_bn_bwd_ws_floats((int64_t)N * H * W, K)}, fopt);
  auto sums = at::empty({2, K}, fopt);
  pdt::launch_pool_bn_bwd_reduce(cbf(dpool), idx.data_ptr<uint8_t>(), cbf(y), stats.data_ptr<float>(), N, H,
                                 W, K, dpool.size(1), dpool.size(2), ws.data_ptr<float>(),
                                 sums.data_ptr<float>(), pg.first, pg.second, cur_stream(y));
  return sums;
}

Tensor pool_bn_bwd_apply(const Tensor& dpool, const Tensor& idx, const Tensor& y, const Tensor& stats,
                         const Tensor& gamma, const Tensor& sums, bool training) {
  check_pool_grad(dpool, idx, y, stats);
  c10::hip::HIPGuard g(y.get_device());
  int N = y.size(0), H = y.size(1), W = y.size(2), K = y.size(3);
  TORCH_CHECK(sums.numel() == 2 * K && gamma.numel() == K, "sums [2, K] / gamma [K]");
  auto dy = at::empty_like(y);
  pdt::launch_pool_bn_bwd_apply(cbf(dpool), idx.data_ptr<uint8_t>(), cbf(y), stats.data_ptr<float>(),
                                gamma.data_ptr<float>(), sums.data_ptr<float>(), training, N, H, W, K,
                                dpool.size(1), dpool.size(2), bf(dy), cur_stream(y));
  return dy;
}

Tensor avgpool_fwd(const Tensor& x) {
  check_bf16_nhwc(x, "x");
  c10::hip::HIPGuard g(x.get_device());
  int N = x.size(0), HW = x.size(1) * x.size(2), C = x.size(3);
  auto y = at::empty({N, C}, x.options().dtype(at::kFloat));
  pdt::launch_avgpool_fwd(cbf(x), y.data_ptr<float>(), N, HW, C, cur_stream(x));
  return y;
}

// dy: fp32 [N, C], or [splits, N, C] split-K partials of the fc dgrad (summed here, in order)
Tensor avgpool_bwd(const Tensor& dy, int64_t H, int64_t W) {
  check_f32(dy, "dy");
  TORCH_CHECK(dy.dim() == 2 || dy.dim() == 3, "avgpool_bwd: dy must be fp32 [N, C] or [splits, N, C]");
  c10::hip::HIPGuard g(dy.get_device());
  const int splits = dy.dim() == 3 ? (int)dy.size(0) : 1;
  int N = dy.size(dy.dim() - 2), C = dy.size(dy.dim() - 1);
  auto dx = at::empty({N, H, W, C}, dy.options().dtype(at::kBFloat16));
  pdt::launch_avgpool_bwd(dy.data_ptr<float>(), bf(dx), N, (int)(H * W), C, cur_stream(dy), splits);
  return dx;
}

// ------------------------------------------------------------ quantisation
Tensor quant_e4m3(const Tensor& x, Tensor state, int64_t slot) {
  check_bf16_nhwc(x, "x");
  check_state(state, slot);
  c10::hip::HIPGuard g(x.get_device());
  auto q = at::empty(x.sizes(), x.options().dtype(at::kByte));
  pdt::launch_quant_e4m3(cbf(x), q.data_ptr<uint8_t>(), x.numel(), state.data_ptr<float>(), (int)slot,
                         cur_stream(x));
  return q;
}

// batched row-wise e4m3 quantization of a flat bf16 weight mirror (table: QRowEntry bytes)
void quant_rows_e4m3(const Tensor& src, Tensor dst, Tensor scale, const Tensor& table, int64_t max_rows) {
  check_cuda(src, "src");
  check_cuda(dst, "dst");
  check_cuda(scale, "scale");
  TORCH_CHECK(src.scalar_type() == at::kBFloat16 && dst.scalar_type() == at::kByte &&
              scale.scalar_type() == at::kFloat && src.numel() == dst.numel(), "quant_rows: bf16 -> uint8");
  TORCH_CHECK(table.is_cuda() && table.scalar_type() == at::kByte && table.is_contiguous(),
              "quant_rows: table must be a device byte tensor");
  const int64_t eb = (int64_t)pdt::quant_rows_entry_bytes();
  TORCH_CHECK(table.numel() % eb == 0, "quant_rows: table size");
  c10::hip::HIPGuard gd(src.get_device());
  pdt::launch_quant_rows_e4m3(cbf(src), dst.data_ptr<uint8_t>(), scale.data_ptr<float>(), table.data_ptr(),
                              (int)(table.numel() / eb), (int)max_rows, cur_stream(src));
}

}  // namespace

void register_bn(py::module_& m) {
  def_op(m, "bn_finalize", &bn_finalize, py::arg("part"), py::arg("count"), py::arg("rm"), py::arg("rv"),
         py::arg("gamma"), py::arg("beta"), py::arg("momentum"), py::arg("eps"), py::arg("grows") = 0);
  def_op(m, "bn_eval_params", &bn_eval_params);
  def_op(m, "bn_act_fwd", &bn_act_fwd, py::arg("y"), py::arg("scale"), py::arg("shift"), py::arg("residual"),
         py::arg("relu"), py::arg("res_scale") = py::none(), py::arg("res_shift") = py::none(),
         py::arg("csum") = py::none());
  def_op(m, "bn_act_fwd_mask", &bn_act_fwd_mask, py::arg("y"), py::arg("scale"), py::arg("shift"),
         py::arg("residual"), py::arg("res_scale") = py::none(), py::arg("res_shift") = py::none());
  def_op(m, "bn_act_fwd_q8", &bn_act_fwd_q8, py::arg("y"), py::arg("scale"), py::arg("shift"), py::arg("residual"),
         py::arg("relu"), py::arg("state"), py::arg("slot"), py::arg("want_mask") = false,
         py::arg("want_z") = true);
  def_op(m, "bn_act_bwd_reduce", &bn_act_bwd_reduce, py::arg("dz"), py::arg("z"), py::arg("y"), py::arg("stats"),
         py::arg("mask"), py::arg("dgamma") = py::none(), py::arg("dbeta") = py::none());
  def_op(m, "bn_act_bwd_apply", &bn_act_bwd_apply, py::arg("dz"), py::arg("z"), py::arg("y"), py::arg("stats"),
         py::arg("gamma"), py::arg("sums"), py::arg("mask"), py::arg("training"), py::arg("want_dres"),
         py::arg("dgamma") = py::none(), py::arg("dbeta") = py::none());
  def_op(m, "bn_act_bwd_apply_q8", &bn_act_bwd_apply_q8, py::arg("dz"), py::arg("z"), py::arg("y"),
         py::arg("stats"), py::arg("gamma"), py::arg("sums"), py::arg("mask"), py::arg("want_dres"),
         py::arg("state"), py::arg("slot"), py::arg("want_dy") = true, py::arg("dgamma") = py::none(),
         py::arg("dbeta") = py::none());
  def_op(m, "bn_fold_weights", &bn_fold_weights, py::arg("wt"), py::arg("stats"), py::arg("gamma"),
         py::arg("sums"), py::arg("count"));
  def_op(m, "bn_fold_wgrad", &bn_fold_wgrad, py::arg("t1"), py::arg("gram"), py::arg("colsum"), py::arg("wt"),
         py::arg("stats"), py::arg("gamma"), py::arg("sums"), py::arg("count"), py::arg("out"),
         py::arg("dgamma") = py::none(), py::arg("dbeta") = py::none(), py::arg("done") = py::none(),
         py::arg("zero_sums") = false);
  m.def("bn_csum_slots", &pdt::bn_csum_slots, "slots of bn_act_fwd's column-sum accumulator");
  m.def("bn_counter_bank", [](uintptr_t stream) {
    return pdt::bn_counter_bank(reinterpret_cast<hipStream_t>(stream));
  }, py::arg("stream"));
  def_op(m, "maxpool_fwd", &maxpool_fwd);
  def_op(m, "maxpool_bwd", &maxpool_bwd);
  def_op(m, "bn_relu_maxpool", &bn_relu_maxpool, py::arg("y"), py::arg("scale"), py::arg("shift"),
         py::arg("argmax_y") = false);
  def_op(m, "pool_bn_bwd_reduce", &pool_bn_bwd_reduce, py::arg("dpool"), py::arg("idx"), py::arg("y"),
         py::arg("stats"), py::arg("dgamma") = py::none(), py::arg("dbeta") = py::none());
  def_op(m, "pool_bn_bwd_apply", &pool_bn_bwd_apply);
  def_op(m, "avgpool_fwd", &avgpool_fwd);
  def_op(m, "avgpool_bwd", &avgpool_bwd);
  def_op(m, "quant_e4m3", &quant_e4m3);
  def_op(m, "quant_rows_e4m3", &quant_rows_e4m3);
  m.def("quant_rows_entry_bytes", []() { return (int64_t)pdt::quant_rows_entry_bytes(); });
  m.def("fp8_state_floats", &pdt::fp8_state_floats);
  m.def("fp8_deq_offset", &pdt::fp8_deq_offset);
}
