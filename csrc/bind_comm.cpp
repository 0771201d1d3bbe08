// Bindings of the communication side: the RCCL and xGMI communicators, the gradient reducer and
// the CU-masked side streams.
#include <stdexcept>
#include <string>

#include "bind_util.h"
#include "comm/rccl_comm.h"
#include "comm/xgmi_comm.h"
#include "ddp/reducer.h"

void register_comm(py::module_& m) {
  m.def("xgmi_force_chunks", &pdt::xgmi_force_chunks, py::arg("n") = -1,
        "test hook: RS -> AG chunks per xGMI bucket (1..4), -1 = the size policy");
  // Stream restricted to `ncu` of the device's CUs, evenly spaced over the CU index space (side
  // streams that should leave the rest of the chip to the critical path).  Returns the raw
  // hipStream_t (wrap with torch.cuda.ExternalStream); it lives until the process exits.
  m.def("cu_masked_stream", [](int device, int ncu) {
    c10::hip::HIPGuard guard((c10::DeviceIndex)device);
    int total = 0;
    if (hipDeviceGetAttribute(&total, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || total <= 0)
      throw std::runtime_error("cu_masked_stream: cannot query the CU count");
    ncu = std::max(1, std::min(ncu, total));
    std::vector<uint32_t> mask((total + 31) / 32, 0u);
    for (int i = 0; i < ncu; ++i) {
      const int cu = (int)((int64_t)i * total / ncu);
      mask[cu / 32] |= 1u << (cu % 32);
    }
    hipStream_t s = nullptr;
    const hipError_t e = hipExtStreamCreateWithCUMask(&s, (uint32_t)mask.size(), mask.data());
    if (e != hipSuccess) throw std::runtime_error(std::string("hipExtStreamCreateWithCUMask: ") + hipGetErrorString(e));
    return reinterpret_cast<uintptr_t>(s);
  }, py::arg("device"), py::arg("ncu"));

  py::class_<pdt::RcclComm, std::shared_ptr<pdt::RcclComm>>(m, "RcclComm")
      .def_static("unique_id", []() { return py::bytes(pdt::RcclComm::unique_id()); })
      .def(py::init([](const std::string& uid, int rank, int world, int device, double init_timeout,
                       double op_timeout, bool exit_on_error, int min_channels, int max_channels) {
             py::gil_scoped_release nogil;  // init polls until every rank joined (or the deadline)
             pdt::RcclOptions o;
             o.init_timeout_s = init_timeout;
             o.op_timeout_s = op_timeout;
             o.exit_on_error = exit_on_error;
             o.min_channels = min_channels;
             o.max_channels = max_channels;
             return std::make_shared<pdt::RcclComm>(uid, rank, world, device, o);
           }),
           py::arg("uid"), py::arg("rank"), py::arg("world"), py::arg("device"),
           py::arg("init_timeout") = 600.0, py::arg("op_timeout") = 600.0,
           py::arg("exit_on_error") = false, py::arg("min_channels") = 0, py::arg("max_channels") = 0)
      .def_property_readonly("rank", &pdt::RcclComm::rank)
      .def_property_readonly("world", &pdt::RcclComm::world)
      .def_property_readonly("device", &pdt::RcclComm::device)
      .def_property_readonly("stream_ptr",
                             [](const pdt::RcclComm& c) { return reinterpret_cast<uintptr_t>(c.stream()); })
      .def("all_reduce", &pdt::RcclComm::all_reduce, py::arg("t"), py::arg("op") = "sum",
           py::arg("wait_current") = true, py::call_guard<py::gil_scoped_release>())
      .def("broadcast", &pdt::RcclComm::broadcast, py::arg("t"), py::arg("root") = 0,
           py::arg("wait_current") = true)
      .def("reduce_scatter", &pdt::RcclComm::reduce_scatter, py::arg("inp"), py::arg("out"),
           py::arg("op") = "sum", py::arg("wait_current") = true)
      .def("all_gather", &pdt::RcclComm::all_gather, py::arg("inp"), py::arg("out"),
           py::arg("wait_current") = true)
      .def("comm_wait_current", &pdt::RcclComm::comm_wait_current)
      .def("current_wait_comm", &pdt::RcclComm::current_wait_comm)
      .def("synchronize", &pdt::RcclComm::synchronize, py::call_guard<py::gil_scoped_release>())
      .def("barrier", &pdt::RcclComm::barrier, py::call_guard<py::gil_scoped_release>())
      .def("abort", &pdt::RcclComm::abort, py::call_guard<py::gil_scoped_release>())
      .def("comm_count", &pdt::RcclComm::comm_count)
      .def_static("version", &pdt::RcclComm::version)
      .def_property_readonly("min_channels", [](const pdt::RcclComm& c) { return c.options().min_channels; })
      .def_property_readonly("max_channels", [](const pdt::RcclComm& c) { return c.options().max_channels; })
      .def("check", &pdt::RcclComm::check)
      .def_property_readonly("healthy", &pdt::RcclComm::healthy)
      .def_property_readonly("error", &pdt::RcclComm::error)
      .def_property_readonly("init_seconds", &pdt::RcclComm::init_seconds)
      .def("inject_delay", &pdt::RcclComm::inject_delay, py::arg("seconds"));

  py::class_<pdt::XgmiComm, std::shared_ptr<pdt::XgmiComm>>(m, "XgmiComm")
      .def(py::init<int, int, int, int64_t, int, double, std::string, int, bool>(), py::arg("rank"),
           py::arg("world"), py::arg("device"), py::arg("numel"), py::arg("nbuckets"), py::arg("timeout") = 600.0,
           py::arg("wire") = "fp32", py::arg("max_blocks") = 16, py::arg("exit_on_error") = false)
      .def_property_readonly("wire", [](const pdt::XgmiComm& c) { return c.wire_bf16() ? "bf16" : "fp32"; })
      .def_property_readonly("max_blocks", &pdt::XgmiComm::max_blocks)
      .def_property_readonly("error_message", &pdt::XgmiComm::error_message)
      .def_property_readonly("rank", &pdt::XgmiComm::rank)
      .def_property_readonly("world", &pdt::XgmiComm::world)
      .def_property_readonly("device", &pdt::XgmiComm::device)
      .def_property_readonly("numel", &pdt::XgmiComm::numel)
      .def_property_readonly("stream_ptr",
                             [](const pdt::XgmiComm& c) { return reinterpret_cast<uintptr_t>(c.stream()); })
      .def("ipc_handles", [](const pdt::XgmiComm& c) { return py::bytes(c.ipc_handles()); })
      .def("open_peers", &pdt::XgmiComm::open_peers, py::arg("handles"))
      .def("link_local", &pdt::XgmiComm::link_local, py::arg("comms"))
      .def("grad_buffer", &pdt::XgmiComm::grad_buffer)
      .def_property_readonly("flags_uncached", &pdt::XgmiComm::flags_uncached)
      .def("reduce_bucket", &pdt::XgmiComm::reduce_bucket, py::arg("bucket"), py::arg("offset"),
           py::arg("count"), py::arg("average") = true)
      .def("reduce_bucket_phases", &pdt::XgmiComm::reduce_bucket_phases, py::arg("bucket"), py::arg("offset"),
           py::arg("count"), py::arg("average"), py::arg("lo"), py::arg("hi"))
      .def("comm_wait_current", &pdt::XgmiComm::comm_wait_current)
      .def("current_wait_comm", &pdt::XgmiComm::current_wait_comm)
      .def("synchronize", &pdt::XgmiComm::synchronize, py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("error_code", &pdt::XgmiComm::error_code)
      .def("check", &pdt::XgmiComm::check);

  py::class_<pdt::Reducer>(m, "Reducer")
      .def(py::init<std::vector<Tensor>, std::vector<Tensor>, std::vector<int64_t>, std::vector<Tensor>,
                    std::shared_ptr<pdt::RcclComm>, py::object, py::object, bool, std::string,
                    std::shared_ptr<pdt::XgmiComm>>(),
           py::arg("params"), py::arg("grad_views"), py::arg("bucket_of_param"),
           py::arg("bucket_flats"), py::arg("comm"), py::arg("py_launch"), py::arg("py_finalize"),
           py::arg("average") = true, py::arg("wire_dtype") = "fp32", py::arg("xgmi") = nullptr)
      .def("prepare_for_backward", &pdt::Reducer::prepare_for_backward,
           py::call_guard<py::gil_scoped_release>())
      .def("mark_ready_external", &pdt::Reducer::mark_ready_external)
      .def("set_enabled", &pdt::Reducer::set_enabled)
      .def_property_readonly("enabled", &pdt::Reducer::enabled)
      .def_property_readonly("num_buckets", &pdt::Reducer::num_buckets)
      .def_property_readonly("iterations", &pdt::Reducer::iterations)
      .def("last_launch_order", &pdt::Reducer::last_launch_order)
      .def("set_timing", &pdt::Reducer::set_timing)
      .def("comm_timing", &pdt::Reducer::comm_timing, py::call_guard<py::gil_scoped_release>())
      .def("set_strict", &pdt::Reducer::set_strict)
      .def("set_aux_stream", &pdt::Reducer::set_aux_stream)
      .def_property_readonly("duplicate_marks", &pdt::Reducer::duplicate_marks)
      .def("set_optimizer", &pdt::Reducer::set_optimizer, py::arg("param_flat"), py::arg("grad_flat"))
      .def("arm_optimizer", [](pdt::Reducer& r, double lr, double mom, double damp, double wd, bool nest, bool first,
                               const std::optional<Tensor>& buf, const std::optional<Tensor>& mirror) {
             r.arm_optimizer(lr, mom, damp, wd, nest, first, buf.has_value() ? *buf : Tensor(),
                             mirror.has_value() ? *mirror : Tensor());
           }, py::arg("lr"), py::arg("momentum"), py::arg("dampening"), py::arg("weight_decay"),
           py::arg("nesterov"), py::arg("first"), py::arg("momentum_buf") = py::none(),
           py::arg("mirror") = py::none())
      .def("arm_lars", &pdt::Reducer::arm_lars, py::arg("table"), py::arg("partials"), py::arg("trust"),
           py::arg("weight_decay"), py::arg("eta"), py::arg("eps"), py::arg("bucket_ranges"))
      .def("optimizer_applied", &pdt::Reducer::optimizer_applied)
      .def("consume_optimizer", &pdt::Reducer::consume_optimizer)
      .def_property_readonly("local", &pdt::Reducer::local);
}
