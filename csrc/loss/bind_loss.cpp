// Python module `pytorch_distributed_tutorials_amd._C_loss`: the binary cross-entropy loss head.
//
// A module of its own because the public surface of `_C` is pinned (tests/golden/c_api.json).  It
// shares bind_util.h's argument plumbing with the `_C` binding sources and carries its own copy of
// the PDT_SYNC_CHECK switch, which bindings.cpp defines for `_C`.
#include <cmath>
#include <cstdlib>
#include <mutex>
#include <stdexcept>
#include <string>

#include "bind_util.h"
#include "loss/bce.h"

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

// The arrival tickets of the kernel's last-block hand-off.  A ticket must be zero when a launch
// starts and the launch leaves it zero, so the words are cleared once, when a device is first used,
// and kept for the life of the process.  Consecutive calls walk a ring of kTickets words: calls
// that overlap on different streams do not share one.  The first call on a device allocates, so it
// cannot be made under stream capture (the trainer's eager warm-up steps come first).
constexpr int kTickets = 64;

uint32_t* next_ticket(const Tensor& like, hipStream_t st) {
  static std::mutex mu;
  // never destroyed: the tensors must not outlive the runtime at process exit
  static auto& ring = *new std::unordered_map<int, std::pair<Tensor, uint64_t>>();
  std::lock_guard<std::mutex> lock(mu);
  const int dev = like.get_device();
  auto it = ring.find(dev);
  if (it == ring.end()) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    TORCH_CHECK(hipStreamIsCapturing(st, &cap) == hipSuccess && cap == hipStreamCaptureStatusNone,
                "bce_with_logits: the first call on a device allocates its tickets and cannot be captured; "
                "call it once eagerly first");
    it = ring.emplace(dev, std::make_pair(at::zeros({kTickets}, like.options().dtype(at::kInt)), 0)).first;
    // this once: the zeros must have landed before a call on another stream draws a ticket
    TORCH_CHECK(hipStreamSynchronize(st) == hipSuccess, "bce_with_logits: clearing the tickets failed");
  }
  const uint64_t slot = it->second.second++ % kTickets;
  return reinterpret_cast<uint32_t*>(it->second.first.data_ptr<int32_t>()) + slot;
}

// (loss, dlogits) of the sigmoid cross entropy against the smoothed target of labels_a, blended
// with that of labels_b by lam (fp32 [N]) when both are given, binarised at target_threshold when
// it is >= 0; mean over all elements, or with sum_classes the sum over classes and mean over rows.
// Every check runs before the launch, and the ones a CPU tensor can fail the same way first.
std::tuple<Tensor, Tensor> bce_with_logits(const Tensor& logits, const Tensor& labels_a,
                                           const std::optional<Tensor>& labels_b, const std::optional<Tensor>& lam,
                                           double label_smoothing, double target_threshold, bool sum_classes) {
  TORCH_CHECK(logits.scalar_type() == at::kFloat, "bce_with_logits: logits must be fp32");
  TORCH_CHECK(logits.dim() == 2 && logits.size(0) > 0 && logits.size(1) > 0, "bce_with_logits: logits must be [N, C]");
  TORCH_CHECK(logits.is_contiguous(), "bce_with_logits: logits must be contiguous");
  const int64_t N = logits.size(0), C = logits.size(1);
  TORCH_CHECK(N < (int64_t(1) << 31) && C < (int64_t(1) << 31), "bce_with_logits: N and C must fit 31 bits");
  const Tensor *lb = opt(labels_b), *lm = opt(lam);
  TORCH_CHECK(!lb == !lm, "bce_with_logits: labels_b and lam go together");
  for (const Tensor* t : {&labels_a, lb})
    TORCH_CHECK(!t || (t->scalar_type() == at::kLong && t->dim() == 1 && t->numel() == N && t->is_contiguous()),
                "bce_with_logits: labels_a / labels_b must be contiguous int64 [N]");
  TORCH_CHECK(!lm || (lm->scalar_type() == at::kFloat && lm->dim() == 1 && lm->numel() == N && lm->is_contiguous()),
              "bce_with_logits: lam must be contiguous fp32 [N]");
  TORCH_CHECK(label_smoothing >= 0.0 && label_smoothing <= 1.0,
              "bce_with_logits: label_smoothing must be in [0, 1], got ", label_smoothing);
  TORCH_CHECK(!std::isnan(target_threshold) && target_threshold < 1.0,
              "bce_with_logits: target_threshold must be below 1 (negative = off), got ", target_threshold);
  for (const Tensor* t : {&logits, &labels_a, lb, lm})
    TORCH_CHECK(!t || (t->is_cuda() && t->get_device() == logits.get_device()),
                "bce_with_logits: every tensor must be a GPU tensor of one device");
  c10::hip::HIPGuard g(logits.get_device());
  hipStream_t st = cur_stream(logits);
  uint32_t* ticket = next_ticket(logits, st);
  const double off = label_smoothing / (double)C, on = 1.0 - label_smoothing + off;
  const double inv_count = sum_classes ? 1.0 / (double)N : 1.0 / ((double)N * (double)C);
  auto loss = at::empty({}, logits.options());
  auto dl = at::empty_like(logits);
  auto ws = at::empty({N}, logits.options().dtype(at::kDouble));
  pdt::loss::launch_bce_with_logits(logits.data_ptr<float>(), labels_a.data_ptr<int64_t>(),
                                    lb ? lb->data_ptr<int64_t>() : nullptr, lm ? lm->data_ptr<float>() : nullptr,
                                    loss.data_ptr<float>(), dl.data_ptr<float>(), ws.data_ptr<double>(), ticket,
                                    (int)N, (int)C, (float)on, (float)off,
                                    target_threshold < 0.0 ? -1.f : (float)target_threshold, inv_count, st);
  return {loss, dl};
}

}  // namespace

PYBIND11_MODULE(_C_loss, m) {
  m.doc() = "MI355X (gfx950) loss heads: fused binary cross entropy with logits (loss and dlogits in one launch)";
  def_op(m, "bce_with_logits", &bce_with_logits, py::arg("logits"), py::arg("labels_a"),
         py::arg("labels_b") = py::none(), py::arg("lam") = py::none(), py::arg("label_smoothing") = 0.0,
         py::arg("target_threshold") = -1.0, py::arg("sum_classes") = false);
  m.def("set_sync_check", [](bool on) { pdt::bind::g_sync_check = on; });
  m.def("sync_check_enabled", []() { return pdt::bind::g_sync_check; });
}
