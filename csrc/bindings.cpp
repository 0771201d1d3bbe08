// Python module of the native extension `pytorch_distributed_tutorials_amd._C`.
//
// The binding sources (bind_*.cpp, one per op family, helpers in bind_util.h) adapt torch tensors to
// the raw-pointer launchers of csrc/kernels (which are compiled without any PyTorch headers),
// allocate outputs/workspaces through the PyTorch caching allocator and launch on the current HIP
// stream, so the ops compose with autograd, streams and graph capture.  bind_comm.cpp exposes the
// RCCL / xGMI communicators and the gradient reducer.
#include <cstdlib>
#include <stdexcept>
#include <string>

#include "bind_util.h"

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

PYBIND11_MODULE(_C, m) {
  m.doc() = "MI355X (gfx950) native kernels, RCCL communicator and DDP reducer";
  register_conv(m);
  register_bn(m);
  register_train(m);
  register_comm(m);
  m.def("set_sync_check", [](bool on) { pdt::bind::g_sync_check = on; });
  m.def("sync_check_enabled", []() { return pdt::bind::g_sync_check; });
}
