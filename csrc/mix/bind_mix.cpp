// Python module `pytorch_distributed_tutorials_amd._C_mix`: the batch-mixing ops (MixUp / CutMix).
//
// A module of its own because the public surface of `_C` is pinned (tests/golden/c_api.json).  It
// shares bind_util.h's argument plumbing with the `_C` binding sources and carries its own copy of
// the PDT_SYNC_CHECK switch, which bindings.cpp defines for `_C`.
#include <cstdlib>
#include <stdexcept>
#include <string>

#include "bind_util.h"
#include "mix/mix.h"

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

// _C.augment's arguments plus partner int64 [B], w fp32 [B], box int32 [B, 4] = (y1, y2, x1, x2)
Tensor augment_mix(const Tensor& images, const Tensor& idx, const Tensor& oy, const Tensor& ox,
                   const std::optional<Tensor>& flip, int64_t pad, bool normalize, std::vector<double> mean,
                   std::vector<double> stdv, const Tensor& partner, const Tensor& w, const Tensor& box) {
  check_cuda(images, "images");
  TORCH_CHECK(images.dim() == 4 && (images.scalar_type() == at::kByte || images.scalar_type() == at::kFloat),
              "images must be uint8 or fp32 NCHW");
  for (const Tensor* t : {&idx, &oy, &ox, &partner})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kLong && t->is_contiguous() && t->numel() == idx.numel(),
                "idx/oy/ox/partner must be device int64 [B]");
  const bool* fp = nullptr;
  if (const Tensor* f = opt(flip)) {
    TORCH_CHECK(f->is_cuda() && f->scalar_type() == at::kBool && f->is_contiguous() && f->numel() == idx.numel(),
                "flip must be device bool [B]");
    fp = f->data_ptr<bool>();
  }
  check_f32(w, "w");
  TORCH_CHECK(w.numel() == idx.numel(), "w must be fp32 [B]");
  check_cuda(box, "box");
  TORCH_CHECK(box.scalar_type() == at::kInt && box.dim() == 2 && box.size(0) == idx.numel() && box.size(1) == 4,
              "box must be int32 [B, 4] (y1, y2, x1, x2)");
  TORCH_CHECK(aligned16(box.data_ptr()), "box must be 16-byte aligned (the kernel loads a row at once)");
  TORCH_CHECK(mean.size() >= (size_t)images.size(1) && stdv.size() >= (size_t)images.size(1), "mean/std per channel");
  TORCH_CHECK(images.size(1) <= 3, "augment_mix: at most 3 channels");
  TORCH_CHECK(images.size(3) % 4 == 0, "augment_mix: width must be a multiple of 4");
  TORCH_CHECK(pad >= 0 && pad < (int64_t(1) << 20), "augment_mix: bad pad");
  c10::hip::HIPGuard g(images.get_device());
  const int B = idx.numel(), C = images.size(1), H = images.size(2), W = images.size(3);
  float m[3] = {0.f, 0.f, 0.f}, sd[3] = {1.f, 1.f, 1.f};
  for (int c = 0; c < C; ++c) { m[c] = (float)mean[c]; sd[c] = (float)stdv[c]; }
  auto out = at::empty({B, C, H, W}, images.options().dtype(at::kFloat));
  pdt::mix::launch_augment_mix(images.data_ptr(), images.scalar_type() == at::kByte, idx.data_ptr<int64_t>(),
                               oy.data_ptr<int64_t>(), ox.data_ptr<int64_t>(), fp, partner.data_ptr<int64_t>(),
                               w.data_ptr<float>(), box.data_ptr<int32_t>(), out.data_ptr<float>(), B, C, H, W,
                               (int)pad, normalize, m, sd, cur_stream(images));
  return out;
}

// (loss, dlogits) against lam * onehot(labels_a) + (1 - lam) * onehot(labels_b); lam fp32 [N]
std::tuple<Tensor, Tensor> softmax_xent_mix(const Tensor& logits_in, const Tensor& labels_a, const Tensor& labels_b,
                                            const Tensor& lam, double label_smoothing) {
  check_cuda(logits_in, "logits");
  TORCH_CHECK(logits_in.dim() == 2 && logits_in.size(0) > 0 && logits_in.size(1) > 0, "logits must be [N, V]");
  TORCH_CHECK(label_smoothing >= 0.0 && label_smoothing <= 1.0, "label_smoothing must be in [0, 1]");
  c10::hip::HIPGuard g(logits_in.get_device());
  Tensor logits = logits_in.scalar_type() == at::kFloat ? logits_in : logits_in.to(at::kFloat);
  const int N = logits.size(0), V = logits.size(1);
  for (const Tensor* t : {&labels_a, &labels_b}) {
    check_cuda(*t, "labels");
    TORCH_CHECK(t->scalar_type() == at::kLong && t->numel() == N, "labels_a/labels_b must be int64 [N]");
  }
  check_f32(lam, "lam");
  TORCH_CHECK(lam.numel() == N, "lam must be fp32 [N]");
  auto loss = at::empty({}, logits.options());
  auto dl = at::empty_like(logits);
  auto ws = at::empty({N}, logits.options());
  pdt::mix::launch_softmax_xent_mix(logits.data_ptr<float>(), labels_a.data_ptr<int64_t>(),
                                    labels_b.data_ptr<int64_t>(), lam.data_ptr<float>(), loss.data_ptr<float>(),
                                    dl.data_ptr<float>(), ws.data_ptr<float>(), N, V, cur_stream(logits),
                                    (float)label_smoothing);
  return {loss, dl};
}

}  // namespace

PYBIND11_MODULE(_C_mix, m) {
  m.doc() = "MI355X (gfx950) batch-mixing kernels: fused MixUp / CutMix augmentation and the two-label loss head";
  def_op(m, "augment_mix", &augment_mix, py::arg("images"), py::arg("idx"), py::arg("oy"), py::arg("ox"),
         py::arg("flip"), py::arg("pad"), py::arg("normalize"), py::arg("mean"), py::arg("std"), py::arg("partner"),
         py::arg("w"), py::arg("box"));
  def_op(m, "softmax_xent_mix", &softmax_xent_mix, py::arg("logits"), py::arg("labels_a"), py::arg("labels_b"),
         py::arg("lam"), py::arg("label_smoothing") = 0.0);
  m.def("set_sync_check", [](bool on) { pdt::bind::g_sync_check = on; });
  m.def("sync_check_enabled", []() { return pdt::bind::g_sync_check; });
}
