// Python module `pytorch_distributed_tutorials_amd._C_opt`: the fused LAMB / AdamW step (optim.LAMB)
// and the device-side gradient-norm clipping that feeds it (optim.clip_grad_norm_).
//
// A module of its own because the public surface of `_C` is pinned (tests/golden/c_api.json).  It
// shares bind_util.h's argument plumbing with the `_C` binding sources and carries its own copy of
// the PDT_SYNC_CHECK switch, which bindings.cpp defines for `_C`.
#include <cmath>
#include <cstdlib>
#include <stdexcept>
#include <string>

#include "bind_util.h"
#include "opt/clip.h"
#include "opt/lamb.h"

namespace pdt::bind {

bool g_sync_check = [] {
  const char* e = std::getenv("PDT_SYNC_CHECK");
  return e && e[0] == '1';
}();

void sync_check(const char* op) {
  if (!g_sync_check) return;
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess)
    throw std::runtime_error(std::string("PDT_SYNC_CHECK: ") + op + ": " + hipGetErrorString(e));
}

}  // namespace pdt::bind

using namespace pdt::bind;
using pdt::opt::LambBufs;
using pdt::opt::LambHyper;
using pdt::opt::LambSpace;

namespace {

// Everything one op works on.  Every check runs here, before any launch, and the ones a CPU tensor
// can fail the same way (dtype, layout, length, table size, segment range, hyperparameters,
// alignment) before the device check.
struct Args {
  LambBufs b;
  LambSpace sp;
  LambHyper h;
};

// the clip record of opt/clip.h
void check_clip_record(const char* op, const Tensor& clip) {
  TORCH_CHECK(clip.scalar_type() == at::kFloat && clip.is_contiguous() && clip.numel() == pdt::opt::kClipRecord, op,
              ": the clip record must be fp32 [", pdt::opt::kClipRecord, "]");
}

// the flat gradient of grad_norm / scale_grads and its record, checked like lamb_args' operands
void clip_args(const char* op, const Tensor& g, const Tensor& clip) {
  TORCH_CHECK(g.scalar_type() == at::kFloat, op, ": the gradient buffer must be fp32");
  TORCH_CHECK(g.is_contiguous() && g.numel() > 0, op, ": the gradient buffer must be contiguous and not empty");
  check_clip_record(op, clip);
  TORCH_CHECK(aligned16(g.data_ptr()), op, ": the gradient buffer must be 16-byte aligned");
}

Args lamb_args(const char* op, const Tensor& p, const Tensor* g, const Tensor& m, const Tensor& v,
               const Tensor& table, const Tensor& partials, const Tensor& trust, const Tensor& rec, int64_t seg_lo,
               int64_t seg_hi, double lr, double beta1, double beta2, double eps, double wd,
               const std::optional<Tensor>& p_bf16, const std::optional<Tensor>& clip = std::nullopt,
               bool trust_clip = false) {
  const Tensor* mir = opt(p_bf16);
  const Tensor* cl = opt(clip);
  for (const Tensor* t : {&p, g, &m, &v}) {
    if (!t) continue;
    TORCH_CHECK(t->scalar_type() == at::kFloat, op, ": param, grad and moment buffers must be fp32");
    TORCH_CHECK(t->is_contiguous(), op, ": flat buffers must be contiguous");
    TORCH_CHECK(t->numel() == p.numel(), op, ": flat buffer length mismatch: ", t->numel(), " against ", p.numel());
  }
  if (mir) {
    TORCH_CHECK(mir->scalar_type() == at::kBFloat16, op, ": p_bf16 must be bf16");
    TORCH_CHECK(mir->is_contiguous() && mir->numel() == p.numel(), op,
                ": bf16 mirror must match the parameter buffer");
  }
  if (cl) check_clip_record(op, *cl);
  TORCH_CHECK(table.scalar_type() == at::kByte && table.is_contiguous(), op, ": table must be a byte tensor");
  TORCH_CHECK(partials.scalar_type() == at::kDouble && partials.is_contiguous() && partials.numel() % 2 == 0, op,
              ": partials must be float64 [nchunks][2]");
  TORCH_CHECK(trust.scalar_type() == at::kFloat && trust.is_contiguous() && trust.numel() > 0, op,
              ": trust must be fp32 [nseg]");
  TORCH_CHECK(rec.scalar_type() == at::kLong && rec.is_contiguous() &&
              rec.numel() * 8 == (int64_t)sizeof(pdt::opt::LambRecord), op, ": the step record must be int64 [",
              sizeof(pdt::opt::LambRecord) / 8, "]");
  const int64_t nseg = trust.numel(), nchunks = partials.numel() / 2;
  TORCH_CHECK(nseg < (int64_t(1) << 30) && nchunks < (int64_t(1) << 30), op, ": table too large");
  TORCH_CHECK(table.numel() == nseg * (int64_t)sizeof(pdt::LarsSeg) + nchunks * (int64_t)sizeof(pdt::LarsChunk), op,
              ": table size does not match trust (segments) and partials (chunks)");
  TORCH_CHECK(0 <= seg_lo && seg_lo < seg_hi && seg_hi <= nseg, op, ": segment range [", seg_lo, ", ", seg_hi,
              ") outside [0, ", nseg, ")");
  TORCH_CHECK(std::isfinite(lr) && lr >= 0.0, op, ": lr must be finite and >= 0, got ", lr);
  TORCH_CHECK(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, op, ": betas must be in [0, 1), got ",
              beta1, ", ", beta2);
  TORCH_CHECK(std::isfinite(eps) && eps >= 0.0 && std::isfinite(wd) && wd >= 0.0, op,
              ": eps and weight_decay must be finite and >= 0");
  Args a;
  a.b = {p.data_ptr<float>(), g ? g->data_ptr<float>() : nullptr, m.data_ptr<float>(), v.data_ptr<float>(),
         mir ? bf(*mir) : nullptr, cl ? cl->data_ptr<float>() : nullptr};
  TORCH_CHECK(aligned16(a.b.p) && aligned16(a.b.g) && aligned16(a.b.m) && aligned16(a.b.v) && aligned16(a.b.mirror) &&
              aligned16(table.data_ptr()) && (reinterpret_cast<uintptr_t>(partials.data_ptr()) & 7) == 0 &&
              (reinterpret_cast<uintptr_t>(rec.data_ptr()) & 7) == 0, op,
              ": flat buffers and the table must be 16-byte aligned");
  for (const Tensor* t : {&p, g, &m, &v, mir, cl, &table, &partials, &trust, &rec})
    TORCH_CHECK(!t || (t->is_cuda() && t->get_device() == p.get_device()), op,
                ": every tensor must be a GPU tensor of one device");
  a.sp.table = table.data_ptr();
  a.sp.nseg = (int)nseg;
  a.sp.nchunks = (int)nchunks;
  a.sp.numel = p.numel();
  a.sp.partials = partials.data_ptr<double>();
  a.sp.trust = trust.data_ptr<float>();
  a.sp.rec = reinterpret_cast<pdt::opt::LambRecord*>(rec.data_ptr());
  a.h = {lr, beta1, beta2, eps, wd, trust_clip};
  return a;
}

// The whole step over the segments [seg_lo, seg_hi) on the current stream: LAMB's three passes, or
// (use_trust off) the AdamW single pass.  `advance`: this call finishes update number done + 1 (the
// last segment range of a step); no allocation, no host read.
void lamb_step(Tensor p, const Tensor& g, Tensor m, Tensor v, const Tensor& table, Tensor partials, Tensor trust,
               Tensor rec, int64_t seg_lo, int64_t seg_hi, double lr, double beta1, double beta2, double eps,
               double wd, bool use_trust, bool advance, const std::optional<Tensor>& p_bf16,
               const std::optional<Tensor>& clip, bool trust_clip) {
  Args a = lamb_args("lamb_step", p, &g, m, v, table, partials, trust, rec, seg_lo, seg_hi, lr, beta1, beta2, eps,
                     wd, p_bf16, clip, trust_clip);
  c10::hip::HIPGuard gd(p.get_device());
  if (use_trust)
    pdt::opt::launch_lamb(a.b, a.sp, (int)seg_lo, (int)seg_hi, a.sp.nchunks, a.h, advance, cur_stream(p));
  else
    pdt::opt::launch_adamw(a.b, a.sp, (int)seg_lo, (int)seg_hi, a.sp.nchunks, a.h, advance, cur_stream(p));
}

// passes 1 and 2 only: the moments, the excluded segments' update and the ratios in `trust`
void lamb_trust(Tensor p, const Tensor& g, Tensor m, Tensor v, const Tensor& table, Tensor partials, Tensor trust,
                Tensor rec, int64_t seg_lo, int64_t seg_hi, double lr, double beta1, double beta2, double eps,
                double wd, bool advance, const std::optional<Tensor>& p_bf16, const std::optional<Tensor>& clip,
                bool trust_clip) {
  Args a = lamb_args("lamb_trust", p, &g, m, v, table, partials, trust, rec, seg_lo, seg_hi, lr, beta1, beta2, eps,
                     wd, p_bf16, clip, trust_clip);
  c10::hip::HIPGuard gd(p.get_device());
  hipStream_t st = cur_stream(p);
  pdt::opt::launch_lamb_moments(a.b, a.sp, (int)seg_lo, (int)seg_hi, a.sp.nchunks, a.h, st);
  pdt::opt::launch_lamb_trust(a.sp, (int)seg_lo, (int)seg_hi, a.h, advance, st);
}

// pass 1 / pass 3 alone (per-pass timing); pass 3 reads the ratios and the record pass 2 left.
// pass 1 writes no ratio: it takes trust_clip for the common signature and makes no use of it.
void lamb_moments(Tensor p, const Tensor& g, Tensor m, Tensor v, const Tensor& table, Tensor partials, Tensor trust,
                  Tensor rec, int64_t seg_lo, int64_t seg_hi, double lr, double beta1, double beta2, double eps,
                  double wd, const std::optional<Tensor>& p_bf16, const std::optional<Tensor>& clip,
                  bool trust_clip) {
  Args a = lamb_args("lamb_moments", p, &g, m, v, table, partials, trust, rec, seg_lo, seg_hi, lr, beta1, beta2,
                     eps, wd, p_bf16, clip, trust_clip);
  c10::hip::HIPGuard gd(p.get_device());
  pdt::opt::launch_lamb_moments(a.b, a.sp, (int)seg_lo, (int)seg_hi, a.sp.nchunks, a.h, cur_stream(p));
}

void lamb_update(Tensor p, const Tensor& m, const Tensor& v, const Tensor& table, Tensor partials, Tensor trust,
                 Tensor rec, int64_t seg_lo, int64_t seg_hi, double lr, double beta1, double beta2, double eps,
                 double wd, const std::optional<Tensor>& p_bf16) {
  Args a = lamb_args("lamb_update", p, nullptr, m, v, table, partials, trust, rec, seg_lo, seg_hi, lr, beta1, beta2,
                     eps, wd, p_bf16);
  c10::hip::HIPGuard gd(p.get_device());
  pdt::opt::launch_lamb_update(a.b, a.sp, (int)seg_lo, (int)seg_hi, a.sp.nchunks, a.h, cur_stream(p));
}

// Passes 1 and 2 of the clipping on the current stream: gpart[c] = float64 sum of squares of the
// c-th 4096-element chunk of g, then clip = (norm, min(max_norm / (norm + 1e-6), 1)).  No host read.
void grad_norm(const Tensor& g, const Tensor& gpart, const Tensor& clip, double max_norm) {
  clip_args("grad_norm", g, clip);
  TORCH_CHECK(gpart.scalar_type() == at::kDouble && gpart.is_contiguous() &&
              gpart.numel() == pdt::opt::clip_chunks(g.numel()), "grad_norm: gpart must be float64 [",
              pdt::opt::clip_chunks(g.numel()), "] (one partial per 4096 elements)");
  TORCH_CHECK(std::isfinite(max_norm) && max_norm > 0.0, "grad_norm: max_norm must be finite and > 0, got ",
              max_norm);
  for (const Tensor* t : {&g, &gpart, &clip})
    TORCH_CHECK(t->is_cuda() && t->get_device() == g.get_device(),
                "grad_norm: every tensor must be a GPU tensor of one device");
  c10::hip::HIPGuard gd(g.get_device());
  pdt::opt::launch_grad_norm(g.data_ptr<float>(), g.numel(), gpart.data_ptr<double>(), clip.data_ptr<float>(),
                             max_norm, cur_stream(g));
}

// g *= clip's coefficient in place; a coefficient of exactly 1 leaves g untouched
void scale_grads(const Tensor& g, const Tensor& clip) {
  clip_args("scale_grads", g, clip);
  for (const Tensor* t : {&g, &clip})
    TORCH_CHECK(t->is_cuda() && t->get_device() == g.get_device(),
                "scale_grads: every tensor must be a GPU tensor of one device");
  c10::hip::HIPGuard gd(g.get_device());
  pdt::opt::launch_scale_grads(g.data_ptr<float>(), g.numel(), clip.data_ptr<float>(), cur_stream(g));
}

}  // namespace

#define LAMB_COMMON                                                                                              \
  py::arg("table"), py::arg("partials"), py::arg("trust"), py::arg("rec"), py::arg("seg_lo"), py::arg("seg_hi"), \
      py::arg("lr"), py::arg("beta1"), py::arg("beta2"), py::arg("eps"), py::arg("weight_decay")

#define CLIP_ARGS py::arg("clip") = py::none(), py::arg("trust_clip") = false

PYBIND11_MODULE(_C_opt, m) {
  m.doc() = "MI355X (gfx950) fused LAMB / AdamW over the flat parameter space";
  def_op(m, "lamb_step", &lamb_step, py::arg("p"), py::arg("g"), py::arg("m"), py::arg("v"), LAMB_COMMON,
         py::arg("use_trust"), py::arg("advance"), py::arg("p_bf16") = py::none(), CLIP_ARGS);
  def_op(m, "lamb_trust", &lamb_trust, py::arg("p"), py::arg("g"), py::arg("m"), py::arg("v"), LAMB_COMMON,
         py::arg("advance"), py::arg("p_bf16") = py::none(), CLIP_ARGS);
  def_op(m, "lamb_moments", &lamb_moments, py::arg("p"), py::arg("g"), py::arg("m"), py::arg("v"), LAMB_COMMON,
         py::arg("p_bf16") = py::none(), CLIP_ARGS);
  def_op(m, "lamb_update", &lamb_update, py::arg("p"), py::arg("m"), py::arg("v"), LAMB_COMMON,
         py::arg("p_bf16") = py::none());
  def_op(m, "grad_norm", &grad_norm, py::arg("g"), py::arg("gpart"), py::arg("clip"), py::arg("max_norm"));
  def_op(m, "scale_grads", &scale_grads, py::arg("g"), py::arg("clip"));
  m.def("record_elems", []() { return (int64_t)(sizeof(pdt::opt::LambRecord) / 8); });
  m.def("set_sync_check", [](bool on) { pdt::bind::g_sync_check = on; });
  m.def("sync_check_enabled", []() { return pdt::bind::g_sync_check; });
}
