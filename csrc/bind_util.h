// Argument plumbing shared by the binding sources (bind_*.cpp): tensor checks, the unpacking of
// optional operands, the side-stream hand-off and op registration.  Everything here is inline and
// allocation-free: the ops run 20-150 times per training step.
#pragma once

#include <ATen/ATen.h>
#include <c10/hip/HIPCachingAllocator.h>
#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/extension.h>

#include <initializer_list>
#include <optional>
#include <tuple>
#include <type_traits>
#include <unordered_map>
#include <utility>
#include <vector>

#include "kernels/kernels.h"

namespace py = pybind11;
using at::Tensor;

// one `void register_<family>(py::module_&)` per binding source, called by bindings.cpp
void register_conv(py::module_& m);
void register_bn(py::module_& m);
void register_train(py::module_& m);
void register_comm(py::module_& m);

namespace pdt::bind {

// ---------------------------------------------------------------- debug mode
// PDT_SYNC_CHECK=1 (or _C.set_sync_check(True)): every op synchronizes the device after its
// launches and turns an asynchronous kernel fault into an exception naming the op that caused
// it (the role CUDA_LAUNCH_BLOCKING / AMD_SERIALIZE_KERNEL play, scoped to this extension).
// Defined in bindings.cpp.
extern bool g_sync_check;
void sync_check(const char* op);

// the one op another family calls (conv_fwd_bn's partials path): defined in bind_bn.cpp
Tensor bn_finalize(const Tensor& part, int64_t count, const Tensor& rm, const Tensor& rv, const Tensor& gamma,
                   const Tensor& beta, double momentum, double eps, int64_t grows_in);

template <typename R, typename... A>
auto checked(const char* op, R (*f)(A...)) {
  return [op, f](A... a) -> R {
    if constexpr (std::is_void_v<R>) {
      f(std::forward<A>(a)...);
      sync_check(op);
    } else {
      R r = f(std::forward<A>(a)...);
      sync_check(op);
      return r;
    }
  };
}

// m.def(name, f, extra...) with f wrapped by checked(name, f)
template <typename F, typename... Extra>
void def_op(py::module_& m, const char* name, F f, const Extra&... extra) {
  m.def(name, checked(name, f), extra...);
}

// ------------------------------------------------------------ tensor checks
inline hipStream_t cur_stream(const Tensor& t) {
  return c10::hip::getCurrentHIPStream(t.get_device()).stream();
}

inline void check_cuda(const Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

inline void check_bf16_nhwc(const Tensor& t, const char* name) {
  check_cuda(t, name);
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, name, " must be bf16");
  TORCH_CHECK(t.dim() == 4, name, " must be 4-D NHWC");
  TORCH_CHECK(t.size(3) % 8 == 0, name, " channels must be a multiple of 8");
  TORCH_CHECK(t.numel() < (int64_t(1) << 30), name, " too large for 32-bit buffer addressing");
}

inline void check_u8_nhwc(const Tensor& t, const char* name) {
  check_cuda(t, name);
  TORCH_CHECK(t.scalar_type() == at::kByte && t.dim() == 4, name, " must be uint8 (fp8 bits) NHWC");
  TORCH_CHECK(t.size(3) % 16 == 0, name, " channels must be a multiple of 16");
  TORCH_CHECK(t.numel() < (int64_t(1) << 31), name, " too large for 32-bit buffer addressing");
}

inline void check_state(const Tensor& st, int64_t slot) {
  check_cuda(st, "fp8 state");
  TORCH_CHECK(st.scalar_type() == at::kFloat && st.numel() == pdt::fp8_state_floats(),
              "fp8 state must be fp32 [fp8_state_floats()]");
  TORCH_CHECK(slot >= 0 && slot < 3, "fp8 slot must be 0..2");
}

inline void check_f32(const Tensor& t, const char* name) {
  check_cuda(t, name);
  TORCH_CHECK(t.scalar_type() == at::kFloat, name, " must be contiguous fp32");
}

// a scalar a kernel reads from device memory
inline const float* dev_scalar(const Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.numel() == 1, name,
              " must be a device fp32 scalar");
  return t.data_ptr<float>();
}

inline void check_stats(const Tensor& stats, int64_t K) {
  TORCH_CHECK(stats.scalar_type() == at::kFloat && stats.numel() == 4 * K && stats.is_contiguous(),
              "stats must be fp32 [4, K]");
}

inline uint16_t* bf(const Tensor& t) { return reinterpret_cast<uint16_t*>(t.data_ptr()); }
inline const uint16_t* cbf(const Tensor& t) { return reinterpret_cast<const uint16_t*>(t.data_ptr()); }

// ---------------------------------------------------------- optional operands
// the tensor of an optional argument, null when it is None or undefined
inline const Tensor* opt(const std::optional<Tensor>& t) {
  return t.has_value() && t->defined() ? &*t : nullptr;
}

// Addend of a dgrad: the full [N,H,W,C] layout of dx (layout 0), or a compact stride-2 map
// [N, ceil(H/2), ceil(W/2), C] that contributes at even (h, w) only (layout 2).
struct Addend {
  const uint16_t* ptr = nullptr;
  int layout = 0;
};

// against dx [s.N, s.H, s.W, s.C], before dx exists (so before the op allocates or launches)
inline Addend dgrad_addend(const std::optional<Tensor>& addend, const pdt::ConvShape& s) {
  const Tensor* a = opt(addend);
  if (!a) return {};
  check_bf16_nhwc(*a, "addend");
  if (a->sizes() == at::IntArrayRef({s.N, s.H, s.W, s.C})) return {cbf(*a), 0};
  TORCH_CHECK(a->size(0) == s.N && a->size(1) == (s.H + 1) / 2 && a->size(2) == (s.W + 1) / 2 &&
              a->size(3) == s.C, "dgrad addend must have the shape of dx or be its stride-2 compact map");
  return {cbf(*a), 2};
}

// optional residual of a BN apply over y
inline const uint16_t* residual_ptr(const std::optional<Tensor>& res, const Tensor& y) {
  const Tensor* r = opt(res);
  if (!r) return nullptr;
  check_bf16_nhwc(*r, "residual");
  TORCH_CHECK(r->sizes() == y.sizes(), "residual shape mismatch");
  return cbf(*r);
}

// optional BN parameter-gradient sinks (fp32 [K], both or neither)
inline std::pair<float*, float*> bn_param_sinks(const std::optional<Tensor>& dgamma,
                                                const std::optional<Tensor>& dbeta, int64_t K) {
  const Tensor* dg = opt(dgamma);
  const Tensor* db = opt(dbeta);
  TORCH_CHECK(!dg == !db, "dgamma and dbeta go together");
  if (!dg) return {nullptr, nullptr};
  TORCH_CHECK(dg->is_contiguous() && db->is_contiguous() && dg->numel() == K && db->numel() == K &&
              dg->scalar_type() == at::kFloat && db->scalar_type() == at::kFloat, "dgamma/dbeta: fp32 [C]");
  return {dg->data_ptr<float>(), db->data_ptr<float>()};
}

// ------------------------------------------------------------------- shapes
inline pdt::ConvShape shape_of(int N, int H, int W, int C, int K, int R, int S, int stride, int pad) {
  pdt::ConvShape s;
  s.N = N; s.H = H; s.W = W; s.C = C; s.K = K; s.R = R; s.S = S;
  s.stride = stride; s.pad = pad;
  s.Ho = (H + 2 * pad - R) / stride + 1;
  s.Wo = (W + 2 * pad - S) / stride + 1;
  return s;
}

// Forward conv of NHWC x (bf16, or the uint8 bits of fp8) with packed weights wk [K,R,S,Cx] of the
// same element type: the shape and the bf16 output.  The caller holds the device guard.
inline std::pair<pdt::ConvShape, Tensor> conv_fwd_prologue(const Tensor& x, const Tensor& wk, int64_t stride,
                                                           int64_t pad, bool fp8) {
  if (fp8) check_u8_nhwc(x, "x");
  else check_bf16_nhwc(x, "x");
  check_cuda(wk, "wk");
  TORCH_CHECK(wk.dim() == 4 && wk.size(3) == x.size(3) && (!fp8 || wk.scalar_type() == at::kByte),
              "packed weight must be [K,R,S,Cx] (uint8 for fp8)");
  auto s = shape_of(x.size(0), x.size(1), x.size(2), x.size(3), wk.size(0), wk.size(1), wk.size(2), stride,
                    pad);
  TORCH_CHECK(s.K % 8 == 0, "output channels must be a multiple of 8");
  return {s, at::empty({s.N, s.Ho, s.Wo, s.K}, x.options().dtype(at::kBFloat16))};
}

// Shape of the dgrad of bf16 dy [N,Ho,Wo,K] through weights w [K,C,R,S] back to x_shape (NHWC)
inline pdt::ConvShape dgrad_prologue(const Tensor& dy, const Tensor& w, const std::vector<int64_t>& xs,
                                     int64_t stride, int64_t pad) {
  check_bf16_nhwc(dy, "dy");
  TORCH_CHECK(xs.size() == 4, "x shape must be NHWC");
  TORCH_CHECK(xs[3] == w.size(1), "dgrad: x channels must equal weight in-channels");
  auto s = shape_of(xs[0], xs[1], xs[2], xs[3], w.size(0), w.size(2), w.size(3), stride, pad);
  TORCH_CHECK(s.Ho == dy.size(1) && s.Wo == dy.size(2) && s.K == dy.size(3), "dgrad: dy shape mismatch");
  return s;
}

// BN backward over dz / y [.., K] with statistics [4, K]: K, the row count M and z for mask 1
struct BnBwd {
  int K;
  int64_t M;
  const uint16_t* z;
};

// pow2_groups: the reduce and the fp8 apply keep one 8-channel group per thread only when K / 8
// divides 256; the bf16 apply rounds its grid to a multiple of K / 8 (ew_blocks) and takes any K % 8 == 0
inline BnBwd bn_bwd_prologue(const Tensor& dz, const Tensor& y, const Tensor& stats, int64_t mask,
                             const Tensor& z, bool pow2_groups = true) {
  check_bf16_nhwc(dz, "dz");
  check_bf16_nhwc(y, "y");
  const int K = y.size(3);
  TORCH_CHECK(!pow2_groups || 256 % (K / 8) == 0, "bn backward: channels must divide 2048 and be a power of two");
  check_stats(stats, K);
  if (mask == 1) check_bf16_nhwc(z, "z");
  return {K, y.numel() / K, mask == 1 ? cbf(z) : nullptr};
}

// --------------------------------------------------------- weight gradients
// A caller-owned weight-gradient accumulator: fp32 [K,C,R,S] whose memory is KRSC-contiguous (a
// channels_last view of the flat gradient buffer)
inline void check_krsc_out(const Tensor& o, int K, int C, int R, int S) {
  TORCH_CHECK(o.scalar_type() == at::kFloat && o.dim() == 4 && o.size(0) == K && o.size(1) == C &&
              o.size(2) == R && o.size(3) == S, "wgrad out: bad shape/dtype");
  // KRSC-dense: strides (RSC, 1, SC, C); a size-1 dim may carry any stride
  const int64_t want[4] = {(int64_t)R * S * C, 1, (int64_t)S * C, (int64_t)C};
  for (int d = 0; d < 4; ++d)
    TORCH_CHECK(o.size(d) == 1 || o.stride(d) == want[d], "wgrad out must be channels_last (KRSC) dense");
}

// Tail of the stem weight gradients: unpack the super-pixel gradient dwsp [K,R,Sp,8] into `out`
// (fp32 [K,C,R,S] of any strides, accumulated into) or into a fresh channels_last tensor
inline Tensor stem_unpack(const Tensor& dwsp, const std::optional<Tensor>& out, int K, int C, int R, int S,
                          int Sp, hipStream_t st) {
  const Tensor* acc = opt(out);
  if (acc)
    TORCH_CHECK(acc->scalar_type() == at::kFloat && acc->dim() == 4 && acc->size(0) == K && acc->size(1) == C &&
                acc->size(2) == R && acc->size(3) == S, "stem wgrad out: bad shape/dtype");
  Tensor o = acc ? *acc : at::empty({K, C, R, S}, dwsp.options().memory_format(at::MemoryFormat::ChannelsLast));
  int64_t os[4] = {o.stride(0), o.stride(1), o.stride(2), o.stride(3)};
  pdt::launch_stem_wgrad_unpack(dwsp.data_ptr<float>(), o.data_ptr<float>(), os, K, C, R, S, Sp, acc != nullptr, st);
  return o;
}

// Hand-off to the weight-gradient side stream (ops/fused.py, ops/streams.py) for the rest of a scope:
// the side stream waits for the work queued so far on the current stream (one reusable event per
// calling thread and device: a wait binds to the record made just before it) and becomes the current
// stream, so workspaces allocated in the scope belong to it.  keep() records operands for the side
// stream so the caching allocator holds their memory until it is done.  Replaces torch's
// wait_stream + stream context + record_stream calls: ~25 us of host issue per weight gradient
// (scripts/host_profile.py), 20-53 of them per step.  side == 0: stays on the current stream.
class SideStream {
 public:
  SideStream(int64_t side, c10::DeviceIndex dev) : stream_(c10::hip::getCurrentHIPStream(dev)) {
    if (side == 0) return;
    // per calling thread (autograd runs a device's backward on one long-lived engine thread) and
    // device; kept for the process lifetime like torch's own stream pool
    static thread_local std::unordered_map<int, hipEvent_t> evs;
    hipEvent_t& ev = evs[(int)dev];
    if (ev == nullptr)
      TORCH_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess, "hipEventCreate failed");
    TORCH_CHECK(hipEventRecord(ev, stream_.stream()) == hipSuccess, "hipEventRecord failed");
    stream_ = c10::hip::getStreamFromExternal(reinterpret_cast<hipStream_t>(side), dev);
    TORCH_CHECK(hipStreamWaitEvent(stream_.stream(), ev, 0) == hipSuccess, "hipStreamWaitEvent failed");
    guard_.emplace(stream_);
  }
  hipStream_t stream() const { return stream_.stream(); }
  void keep(std::initializer_list<const Tensor*> operands) const {
    if (!guard_) return;
    for (const Tensor* t : operands) c10::hip::HIPCachingAllocator::recordStream(t->storage().data_ptr(), stream_);
  }

 private:
  c10::hip::HIPStream stream_;
  std::optional<c10::hip::HIPStreamGuard> guard_;
};

// ------------------------------------------------------ flat optimizer buffers
inline bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// fp32 parameter / gradient buffers of one size
inline void check_flat_pair(const Tensor& p, const Tensor& g) {
  check_cuda(p, "param");
  check_cuda(g, "grad");
  TORCH_CHECK(p.scalar_type() == at::kFloat && g.scalar_type() == at::kFloat, "fp32 flat buffers only");
  TORCH_CHECK(p.numel() == g.numel(), "param/grad size mismatch");
}

// Operands of a fused optimizer step over the flat space: p, g, the momentum buffer (required when
// momentum != 0, ignored otherwise: momentum 0 passes None) and the optional bf16 mirror of p.
// All of one size and 16-byte aligned (the kernels move 4-element vectors).
struct FlatArgs {
  float* p;
  const float* g;
  float* buf;
  uint16_t* mirror;
};

inline FlatArgs flat_opt_args(const char* op, const Tensor& p, const Tensor& g,
                              const std::optional<Tensor>& buf_opt, double momentum,
                              const std::optional<Tensor>& p_bf16) {
  check_flat_pair(p, g);
  FlatArgs a{p.data_ptr<float>(), g.data_ptr<float>(), nullptr, nullptr};
  if (momentum != 0.0) {
    const Tensor* buf = opt(buf_opt);
    TORCH_CHECK(buf, op, ": momentum != 0 needs a momentum buffer");
    check_cuda(*buf, "momentum_buffer");
    TORCH_CHECK(buf->scalar_type() == at::kFloat && buf->numel() == p.numel(), "momentum buffer size mismatch");
    a.buf = buf->data_ptr<float>();
  }
  if (const Tensor* m = opt(p_bf16)) {
    check_cuda(*m, "p_bf16");
    TORCH_CHECK(m->scalar_type() == at::kBFloat16 && m->numel() == p.numel(), op,
                ": bf16 mirror must match the parameter buffer");
    a.mirror = bf(*m);
  }
  TORCH_CHECK(aligned16(a.p) && aligned16(a.g) && aligned16(a.buf) && aligned16(a.mirror), op,
              ": flat buffers must be 16-byte aligned");
  return a;
}

}  // namespace pdt::bind
