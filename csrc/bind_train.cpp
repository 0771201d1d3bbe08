// Bindings of what surrounds the network in a training step: the input augmentation, the fc layer,
// the loss head and the fused optimizers (SGD, LARS) over the flat parameter space.
#include "bind_util.h"

using namespace pdt::bind;

namespace {

// ---------------------------------------------------------------- augment
// images: uint8 or fp32 [N,C,H,W] (device); idx/oy/ox int64 [B]; flip bool [B] or None
Tensor augment(const Tensor& images, const Tensor& idx, const Tensor& oy, const Tensor& ox,
               const std::optional<Tensor>& flip, int64_t pad, bool normalize, std::vector<double> mean,
               std::vector<double> stdv) {
  check_cuda(images, "images");
  TORCH_CHECK(images.dim() == 4 && (images.scalar_type() == at::kByte || images.scalar_type() == at::kFloat),
              "images must be uint8 or fp32 NCHW");
  for (const Tensor* t : {&idx, &oy, &ox})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kLong && t->is_contiguous() && t->numel() == idx.numel(),
                "idx/oy/ox must be device int64 [B]");
  const bool* fp = nullptr;
  if (const Tensor* f = opt(flip)) {
    TORCH_CHECK(f->is_cuda() && f->scalar_type() == at::kBool && f->numel() == idx.numel(),
                "flip must be device bool [B]");
    fp = f->data_ptr<bool>();
  }
  TORCH_CHECK(mean.size() >= (size_t)images.size(1) && stdv.size() >= (size_t)images.size(1), "mean/std per channel");
  c10::hip::HIPGuard g(images.get_device());
  const int B = idx.numel(), C = images.size(1), H = images.size(2), W = images.size(3);
  float m[3] = {0.f, 0.f, 0.f}, sd[3] = {1.f, 1.f, 1.f};
  for (int c = 0; c < C; ++c) { m[c] = (float)mean[c]; sd[c] = (float)stdv[c]; }
  auto out = at::empty({B, C, H, W}, images.options().dtype(at::kFloat));
  pdt::launch_augment(images.data_ptr(), images.scalar_type() == at::kByte, idx.data_ptr<int64_t>(),
                      oy.data_ptr<int64_t>(), ox.data_ptr<int64_t>(), fp, out.data_ptr<float>(), B, C, H, W,
                      (int)pad, normalize, m, sd, cur_stream(images));
  return out;
}

// ---------------------------------------------------------------------- fc
// logits[N][V] = pooled[N][C] . W[V][C]^T + b
Tensor fc_forward(const Tensor& pooled, const Tensor& w, const Tensor& b) {
  check_f32(pooled, "pooled"); check_f32(w, "weight"); check_f32(b, "bias");
  TORCH_CHECK(pooled.dim() == 2 && w.dim() == 2 && w.size(1) == pooled.size(1) && b.numel() == w.size(0),
              "fc_forward: pooled [N, C], weight [V, C], bias [V]");
  c10::hip::HIPGuard g(pooled.get_device());
  const int N = pooled.size(0), C = pooled.size(1), V = w.size(0);
  auto out = at::empty({N, V}, pooled.options());
  pdt::FcArgs a{};
  a.a = pooled.data_ptr<float>(); a.b = w.data_ptr<float>(); a.c = out.data_ptr<float>();
  a.bias = b.data_ptr<float>();
  a.M = N; a.N = V; a.K = C; a.sam = C; a.sak = 1; a.sbn = C; a.sbk = 1; a.ldc = V;
  a.splits = pdt::fc_splits(N, V, C);
  a.kper = (C + a.splits - 1) / a.splits;
  a.kper = (a.kper + 31) / 32 * 32;
  a.splits = (C + a.kper - 1) / a.kper;
  Tensor ws;
  if (a.splits > 1) {
    ws = at::empty({a.splits, N, V}, pooled.options());
    a.ws = ws.data_ptr<float>();
  }
  hipStream_t st = cur_stream(pooled);
  pdt::launch_fc_gemm(a, st);
  if (a.splits > 1) pdt::launch_fc_splitk_reduce(a.ws, a.splits, N, V, a.bias, a.c, V, st);
  return out;
}

// Backward of the fc: returns (dpooled partials [splits, N, C] for avgpool_bwd, dW, db).  dW / db
// accumulate into `dw_out` / `db_out` when given (flat gradient views), else come back fresh.
std::tuple<Tensor, Tensor, Tensor> fc_backward(const Tensor& dlogits, const Tensor& pooled, const Tensor& w,
                                               const std::optional<Tensor>& dw_out,
                                               const std::optional<Tensor>& db_out) {
  check_f32(dlogits, "dlogits"); check_f32(pooled, "pooled"); check_f32(w, "weight");
  const int N = dlogits.size(0), V = dlogits.size(1), C = pooled.size(1);
  TORCH_CHECK(pooled.size(0) == N && w.size(0) == V && w.size(1) == C, "fc_backward: shape mismatch");
  c10::hip::HIPGuard g(dlogits.get_device());
  hipStream_t st = cur_stream(dlogits);
  const Tensor* acc_w = opt(dw_out);
  const Tensor* acc_b = opt(db_out);
  if (acc_w)
    TORCH_CHECK(acc_w->scalar_type() == at::kFloat && acc_w->numel() == (int64_t)V * C &&
                acc_w->stride(0) == C && acc_w->stride(1) == 1, "dw_out must be fp32 [V, C] row-major");
  Tensor dw = acc_w ? *acc_w : at::empty({V, C}, w.options());
  if (acc_b)
    TORCH_CHECK(acc_b->scalar_type() == at::kFloat && acc_b->numel() == V && acc_b->is_contiguous(),
                "db_out must be contiguous fp32 [V]");
  Tensor db = acc_b ? *acc_b : at::empty({V}, w.options());
  // dW[V][C] (+)= dlogits^T . pooled: A(m = v, k = n) = dlogits[n][v], B(k = n, n = c) = pooled[n][c]
  pdt::FcArgs a{};
  a.a = dlogits.data_ptr<float>(); a.b = pooled.data_ptr<float>(); a.c = dw.data_ptr<float>();
  a.M = V; a.N = C; a.K = N; a.sam = 1; a.sak = V; a.sbn = 1; a.sbk = C; a.ldc = C;
  a.splits = 1; a.kper = N; a.accumulate = acc_w ? 1 : 0;
  if (!acc_w == !acc_b) {  // db from the same pass (shares the accumulate flag)
    a.db = db.data_ptr<float>();
    pdt::launch_fc_gemm(a, st);
  } else {
    pdt::launch_fc_gemm(a, st);
    pdt::launch_fc_colsum(dlogits.data_ptr<float>(), N, V, nullptr, db.data_ptr<float>(), acc_b != nullptr, st);
  }
  // dpooled[N][C] = dlogits . W: A(m = n, k = v) = dlogits[n][v], B(k = v, n = c) = W[v][c]
  pdt::FcArgs d{};
  d.a = dlogits.data_ptr<float>(); d.b = w.data_ptr<float>();
  d.M = N; d.N = C; d.K = V; d.sam = V; d.sak = 1; d.sbn = 1; d.sbk = C; d.ldc = C;
  d.splits = pdt::fc_splits(N, C, V);
  d.kper = ((V + d.splits - 1) / d.splits + 31) / 32 * 32;
  d.splits = (V + d.kper - 1) / d.kper;
  auto dp = at::empty({d.splits, N, C}, dlogits.options());
  if (d.splits > 1) d.ws = dp.data_ptr<float>();
  else d.c = dp.data_ptr<float>();
  pdt::launch_fc_gemm(d, st);
  return {dp, dw, db};
}

// -------------------------------------------------------------------- head
std::tuple<Tensor, Tensor> softmax_xent(const Tensor& logits_in, const Tensor& labels, double label_smoothing) {
  check_cuda(logits_in, "logits");
  TORCH_CHECK(label_smoothing >= 0.0 && label_smoothing <= 1.0, "label_smoothing must be in [0, 1]");
  c10::hip::HIPGuard g(logits_in.get_device());
  Tensor logits = logits_in.scalar_type() == at::kFloat ? logits_in : logits_in.to(at::kFloat);
  TORCH_CHECK(labels.scalar_type() == at::kLong, "labels must be int64");
  int N = logits.size(0), V = logits.size(1);
  auto loss = at::empty({}, logits.options());
  auto dl = at::empty_like(logits);
  auto ws = at::empty({N}, logits.options());
  pdt::launch_softmax_xent(logits.data_ptr<float>(), labels.data_ptr<int64_t>(), loss.data_ptr<float>(),
                           dl.data_ptr<float>(), ws.data_ptr<float>(), N, V, cur_stream(logits),
                           (float)label_smoothing);
  return {loss, dl};
}

// x * alpha for a device scalar alpha (the upstream gradient of the loss), fp32
Tensor scale_by(const Tensor& x, const Tensor& alpha) {
  check_f32(x, "x");
  const float* ap = dev_scalar(alpha, "alpha");
  c10::hip::HIPGuard g(x.get_device());
  auto y = at::empty_like(x);
  pdt::launch_scale(x.data_ptr<float>(), ap, y.data_ptr<float>(), x.numel(), cur_stream(x));
  return y;
}

void add_one_i64(Tensor x) {
  check_cuda(x, "x");
  TORCH_CHECK(x.scalar_type() == at::kLong, "add_one_i64: contiguous int64");
  c10::hip::HIPGuard g(x.get_device());
  pdt::launch_add_one_i64(x.data_ptr<int64_t>(), x.numel(), cur_stream(x));
}

Tensor top1_correct(const Tensor& logits_in, const Tensor& labels) {
  check_cuda(logits_in, "logits");
  c10::hip::HIPGuard g(logits_in.get_device());
  Tensor logits = logits_in.scalar_type() == at::kFloat ? logits_in : logits_in.to(at::kFloat);
  int N = logits.size(0), V = logits.size(1);
  auto cnt = at::empty({}, labels.options().dtype(at::kLong));
  pdt::launch_top1(logits.data_ptr<float>(), labels.data_ptr<int64_t>(), cnt.data_ptr<int64_t>(), N, V,
                   cur_stream(logits));
  return cnt;
}

// --------------------------------------------------------------------- sgd
void sgd_step(Tensor p, const Tensor& g, const std::optional<Tensor>& buf, double lr, double momentum,
              double dampening, double wd, bool nesterov, bool first, double grad_scale,
              const std::optional<Tensor>& p_bf16) {
  FlatArgs a = flat_opt_args("sgd_step", p, g, buf, momentum, p_bf16);
  c10::hip::HIPGuard gd(p.get_device());
  pdt::launch_sgd(a.p, a.g, a.buf, p.numel(), (float)lr, (float)momentum, (float)dampening, (float)wd, nesterov,
                  first, (float)grad_scale, cur_stream(p), a.mirror);
}

// -------------------------------------------------------------------- lars
// table: device bytes, trust.numel() segment entries then partials.numel()/2 chunk entries
// (optim/lars.py builds it); partials: float64 [nchunks][2]; trust: fp32 [nseg]
pdt::LarsSpace lars_space(const Tensor& table, const Tensor& partials, const Tensor& trust, int64_t numel,
                          int64_t seg_lo, int64_t seg_hi) {
  check_cuda(table, "table");
  check_cuda(partials, "partials");
  check_cuda(trust, "trust");
  TORCH_CHECK(table.scalar_type() == at::kByte, "lars: table must be a device byte tensor");
  TORCH_CHECK(partials.scalar_type() == at::kDouble && partials.numel() % 2 == 0,
              "lars: partials must be float64 [nchunks][2]");
  TORCH_CHECK(trust.scalar_type() == at::kFloat && trust.numel() > 0, "lars: trust must be fp32 [nseg]");
  const int64_t nseg = trust.numel(), nchunks = partials.numel() / 2;
  TORCH_CHECK(nseg < (int64_t(1) << 30) && nchunks < (int64_t(1) << 30), "lars: table too large");
  TORCH_CHECK(table.numel() == nseg * (int64_t)pdt::lars_entry_bytes() +
                                   nchunks * (int64_t)pdt::lars_chunk_entry_bytes(),
              "lars: table size does not match trust (segments) and partials (chunks)");
  TORCH_CHECK(aligned16(table.data_ptr()) && (reinterpret_cast<uintptr_t>(partials.data_ptr()) & 7) == 0,
              "lars: table alignment");
  TORCH_CHECK(0 <= seg_lo && seg_lo <= seg_hi && seg_hi <= nseg, "lars: segment range [", seg_lo, ", ", seg_hi,
              ") outside [0, ", nseg, ")");
  pdt::LarsSpace sp;
  sp.table = table.data_ptr();
  sp.nseg = (int)nseg;
  sp.nchunks = (int)nchunks;
  sp.numel = numel;
  sp.partials = partials.data_ptr<double>();
  sp.trust = trust.data_ptr<float>();
  return sp;
}

void lars_trust(const Tensor& p, const Tensor& g, const Tensor& table, Tensor partials, Tensor trust,
                int64_t seg_lo, int64_t seg_hi, double wd, double eta, double eps) {
  check_flat_pair(p, g);
  pdt::LarsSpace sp = lars_space(table, partials, trust, p.numel(), seg_lo, seg_hi);
  c10::hip::HIPGuard gd(p.get_device());
  hipStream_t st = cur_stream(p);
  pdt::launch_lars_norms(p.data_ptr<float>(), g.data_ptr<float>(), sp, (int)seg_lo, (int)seg_hi, sp.nchunks, st);
  pdt::launch_lars_trust(sp, (int)seg_lo, (int)seg_hi, wd, eta, eps, st);
}

// the passes of lars_trust one at a time (per-pass timing)
void lars_norms(const Tensor& p, const Tensor& g, const Tensor& table, Tensor partials, Tensor trust,
                int64_t seg_lo, int64_t seg_hi) {
  check_flat_pair(p, g);
  pdt::LarsSpace sp = lars_space(table, partials, trust, p.numel(), seg_lo, seg_hi);
  c10::hip::HIPGuard gd(p.get_device());
  pdt::launch_lars_norms(p.data_ptr<float>(), g.data_ptr<float>(), sp, (int)seg_lo, (int)seg_hi, sp.nchunks,
                         cur_stream(p));
}

void lars_trust_only(const Tensor& table, Tensor partials, Tensor trust, int64_t seg_lo, int64_t seg_hi,
                     double wd, double eta, double eps) {
  pdt::LarsSpace sp = lars_space(table, partials, trust, 0, seg_lo, seg_hi);
  c10::hip::HIPGuard gd(trust.get_device());
  pdt::launch_lars_trust(sp, (int)seg_lo, (int)seg_hi, wd, eta, eps, cur_stream(trust));
}

void lars_step(Tensor p, const Tensor& g, const std::optional<Tensor>& buf, const Tensor& table,
               Tensor partials, Tensor trust, int64_t seg_lo, int64_t seg_hi, double lr, double momentum,
               double dampening, double wd, bool nesterov, bool first, double eta, double eps,
               const std::optional<Tensor>& p_bf16) {
  FlatArgs a = flat_opt_args("lars_step", p, g, buf, momentum, p_bf16);
  pdt::LarsSpace sp = lars_space(table, partials, trust, p.numel(), seg_lo, seg_hi);
  c10::hip::HIPGuard gd(p.get_device());
  pdt::launch_lars(a.p, a.g, a.buf, sp, (int)seg_lo, (int)seg_hi, sp.nchunks, (float)lr, (float)momentum,
                   (float)dampening, wd, nesterov, first, eta, eps, cur_stream(p), a.mirror);
}

// the update pass alone, with the trust ratios already in `trust` (diagnostics / per-pass timing)
void lars_update(Tensor p, const Tensor& g, const std::optional<Tensor>& buf, const Tensor& table,
                 Tensor partials, Tensor trust, int64_t seg_lo, int64_t seg_hi, double lr, double momentum,
                 double dampening, double wd, bool nesterov, bool first, const std::optional<Tensor>& p_bf16) {
  FlatArgs a = flat_opt_args("lars_update", p, g, buf, momentum, p_bf16);
  pdt::LarsSpace sp = lars_space(table, partials, trust, p.numel(), seg_lo, seg_hi);
  c10::hip::HIPGuard gd(p.get_device());
  pdt::launch_lars_update(a.p, a.g, a.buf, sp, (int)seg_lo, (int)seg_hi, sp.nchunks, (float)lr, (float)momentum,
                          (float)dampening, (float)wd, nesterov, first, cur_stream(p), a.mirror);
}

int64_t lars_entry_bytes() { return (int64_t)pdt::lars_entry_bytes(); }
int64_t lars_chunk_entry_bytes() { return (int64_t)pdt::lars_chunk_entry_bytes(); }
int64_t lars_chunk_elems() { return (int64_t)pdt::lars_chunk_elems(); }

}  // namespace

void register_train(py::module_& m) {
  def_op(m, "augment", &augment, py::arg("images"), py::arg("idx"), py::arg("oy"), py::arg("ox"), py::arg("flip"),
         py::arg("pad"), py::arg("normalize"), py::arg("mean"), py::arg("std"));
  def_op(m, "fc_forward", &fc_forward, py::arg("pooled"), py::arg("weight"), py::arg("bias"));
  def_op(m, "fc_backward", &fc_backward, py::arg("dlogits"), py::arg("pooled"), py::arg("weight"),
         py::arg("dw_out") = py::none(), py::arg("db_out") = py::none());
  def_op(m, "scale_by", &scale_by, py::arg("x"), py::arg("alpha"));
  def_op(m, "add_one_i64", &add_one_i64, py::arg("x"));
  def_op(m, "softmax_xent", &softmax_xent, py::arg("logits"), py::arg("labels"), py::arg("label_smoothing") = 0.0);
  def_op(m, "top1_correct", &top1_correct);
  def_op(m, "sgd_step", &sgd_step, py::arg("p"), py::arg("g"), py::arg("buf"), py::arg("lr"), py::arg("momentum"),
         py::arg("dampening"), py::arg("wd"), py::arg("nesterov"), py::arg("first"), py::arg("grad_scale"),
         py::arg("p_bf16") = py::none());
  def_op(m, "lars_step", &lars_step, py::arg("p"), py::arg("g"), py::arg("buf"), py::arg("table"),
         py::arg("partials"), py::arg("trust"), py::arg("seg_lo"), py::arg("seg_hi"), py::arg("lr"),
         py::arg("momentum"), py::arg("dampening"), py::arg("weight_decay"), py::arg("nesterov"), py::arg("first"),
         py::arg("eta"), py::arg("eps"), py::arg("p_bf16") = py::none());
  def_op(m, "lars_trust", &lars_trust, py::arg("p"), py::arg("g"), py::arg("table"), py::arg("partials"),
         py::arg("trust"), py::arg("seg_lo"), py::arg("seg_hi"), py::arg("weight_decay"), py::arg("eta"),
         py::arg("eps"));
  def_op(m, "lars_update", &lars_update, py::arg("p"), py::arg("g"), py::arg("buf"), py::arg("table"),
         py::arg("partials"), py::arg("trust"), py::arg("seg_lo"), py::arg("seg_hi"), py::arg("lr"),
         py::arg("momentum"), py::arg("dampening"), py::arg("weight_decay"), py::arg("nesterov"), py::arg("first"),
         py::arg("p_bf16") = py::none());
  def_op(m, "lars_norms", &lars_norms, py::arg("p"), py::arg("g"), py::arg("table"), py::arg("partials"),
         py::arg("trust"), py::arg("seg_lo"), py::arg("seg_hi"));
  def_op(m, "lars_trust_only", &lars_trust_only, py::arg("table"), py::arg("partials"), py::arg("trust"),
         py::arg("seg_lo"), py::arg("seg_hi"), py::arg("weight_decay"), py::arg("eta"), py::arg("eps"));
  m.def("lars_entry_bytes", &lars_entry_bytes);
  m.def("lars_chunk_entry_bytes", &lars_chunk_entry_bytes);
  m.def("lars_chunk_elems", &lars_chunk_elems);
}
