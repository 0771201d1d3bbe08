// Python module `pytorch_distributed_tutorials_amd._C_ema`: the weight-EMA update (optim.ModelEma).
//
// A module of its own because the public surface of `_C` is pinned (tests/golden/c_api.json).  It
// shares bind_util.h's argument plumbing with the `_C` binding sources and carries its own copy of
// the PDT_SYNC_CHECK switch, which bindings.cpp defines for `_C`.
#include <cmath>
#include <cstdlib>
#include <stdexcept>
#include <string>

#include "bind_util.h"
#include "ema/ema.h"

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

namespace {

// one averaged fp32 range: dtype, contiguity, length and the alignment rule of the kernel
pdt::ema::LerpSeg lerp_seg(const Tensor& e, const Tensor& p, const Tensor* bf16, const char* what) {
  TORCH_CHECK(e.scalar_type() == at::kFloat && p.scalar_type() == at::kFloat, "ema_update: ", what,
              " buffers must be fp32");
  TORCH_CHECK(e.is_contiguous() && p.is_contiguous(), "ema_update: ", what, " buffers must be contiguous");
  TORCH_CHECK(e.numel() == p.numel(), "ema_update: ", what, " length mismatch: the EMA holds ", e.numel(),
              " elements, the model ", p.numel());
  pdt::ema::LerpSeg s;
  s.e = e.data_ptr<float>();
  s.p = p.data_ptr<float>();
  s.n = e.numel();
  if (bf16) {
    TORCH_CHECK(bf16->scalar_type() == at::kBFloat16, "ema_update: ema_krsc must be bf16");
    TORCH_CHECK(bf16->is_contiguous(), "ema_update: ema_krsc must be contiguous");
    TORCH_CHECK(bf16->numel() == e.numel(), "ema_update: ema_krsc length mismatch: ", bf16->numel(), " against ",
                e.numel());
    s.bf = bf(*bf16);
  }
  if (const char* err = pdt::ema::lerp_seg_error(s)) TORCH_CHECK(false, "ema_update: ", what, ": ", err);
  return s;
}

// e <- e + w * (p - e) over the flat parameters (with the twin's bf16 KRSC mirror as a side output),
// the same over the flat fp32 buffers, and a copy of the flat int64 buffers: one launch on the
// current stream, no allocation, no host read.  Every check runs before the launch, and the ones a
// CPU tensor can fail the same way (dtype, layout, length, w, alignment) before the device check.
void ema_update(const Tensor& ema_flat, const Tensor& param_flat, double w, const std::optional<Tensor>& ema_krsc,
                const std::optional<Tensor>& ema_buf, const std::optional<Tensor>& model_buf,
                const std::optional<Tensor>& ema_int, const std::optional<Tensor>& model_int) {
  TORCH_CHECK(std::isfinite(w) && w >= 0.0 && w <= 1.0, "ema_update: w = 1 - decay must be in [0, 1], got ", w);
  pdt::ema::LerpSeg ps = lerp_seg(ema_flat, param_flat, opt(ema_krsc), "parameter");
  pdt::ema::LerpSeg bs;
  const Tensor *eb = opt(ema_buf), *mb = opt(model_buf);
  TORCH_CHECK(!eb == !mb, "ema_update: ema_buf and model_buf go together");
  if (eb) bs = lerp_seg(*eb, *mb, nullptr, "float-buffer");
  pdt::ema::CopySeg cs;
  const Tensor *ei = opt(ema_int), *mi = opt(model_int);
  TORCH_CHECK(!ei == !mi, "ema_update: ema_int and model_int go together");
  if (ei) {
    TORCH_CHECK(ei->scalar_type() == at::kLong && mi->scalar_type() == at::kLong,
                "ema_update: integer buffers must be int64");
    TORCH_CHECK(ei->is_contiguous() && mi->is_contiguous(), "ema_update: integer buffers must be contiguous");
    TORCH_CHECK(ei->numel() == mi->numel(), "ema_update: integer-buffer length mismatch: ", ei->numel(), " against ",
                mi->numel());
    cs.dst = ei->data_ptr<int64_t>();
    cs.src = mi->data_ptr<int64_t>();
    cs.n = ei->numel();
  }
  for (const Tensor* t : {&ema_flat, &param_flat, opt(ema_krsc), eb, mb, ei, mi})
    TORCH_CHECK(!t || (t->is_cuda() && t->get_device() == ema_flat.get_device()),
                "ema_update: every tensor must be a GPU tensor of one device");
  c10::hip::HIPGuard g(ema_flat.get_device());
  pdt::ema::launch_ema_update(ps, bs, cs, (float)w, cur_stream(ema_flat));
}

}  // namespace

PYBIND11_MODULE(_C_ema, m) {
  m.doc() = "MI355X (gfx950) weight EMA: one fused update over the flat parameters, buffers and counters";
  def_op(m, "ema_update", &ema_update, py::arg("ema_flat"), py::arg("param_flat"), py::arg("w"),
         py::arg("ema_krsc") = py::none(), py::arg("ema_buf") = py::none(), py::arg("model_buf") = py::none(),
         py::arg("ema_int") = py::none(), py::arg("model_int") = py::none());
  m.def("set_sync_check", [](bool on) { pdt::bind::g_sync_check = on; });
  m.def("sync_check_enabled", []() { return pdt::bind::g_sync_check; });
}
