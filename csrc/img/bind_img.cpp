// Python module `pytorch_distributed_tutorials_amd._C_img`: the resampling input transform
// (RandomResizedCrop / centre crop + resize) and the fused augmentation policy (TrivialAugmentWide +
// RandomErasing).
//
// A module of its own because the public surface of `_C` is pinned (tests/golden/c_api.json).  It
// shares bind_util.h's argument plumbing with the `_C` binding sources and carries its own copy of
// the PDT_SYNC_CHECK switch, which bindings.cpp defines for `_C`.
#include <cstdlib>
#include <stdexcept>
#include <string>

#include "bind_util.h"
#include "img/autoaug.h"
#include "img/resample.h"

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

// every row of a host int32 [B, 4] box tensor lies inside an H x W image and is not empty
void check_boxes(const Tensor& box, int64_t H, int64_t W) {
  const int32_t* p = box.data_ptr<int32_t>();
  for (int64_t b = 0; b < box.size(0); ++b, p += 4) {
    const int64_t y0 = p[0], x0 = p[1], h = p[2], w = p[3];
    TORCH_CHECK(h >= 1 && w >= 1 && y0 >= 0 && x0 >= 0 && y0 + h <= H && x0 + w <= W, "resized_crop: box ", b,
                " = (y0 ", y0, ", x0 ", x0, ", h ", h, ", w ", w, ") is empty or reaches outside the ", H, " x ", W,
                " image");
  }
}

// images uint8 / fp32 [N, C, H, W]; idx int64 [B]; box int32 [B, 4] = (y0, x0, h, w) on the device or
// on the host; flip bool [B] or None.  A host box is checked here, row by row, and then uploaded.  A
// device box cannot be read without stalling the stream: the kernel clamps it into the image, and
// with PDT_SYNC_CHECK on (every op synchronizes anyway) it is copied back and checked as well.
Tensor resized_crop(const Tensor& images, const Tensor& idx, const Tensor& box_in, const std::optional<Tensor>& flip,
                    int64_t out_h, int64_t out_w, bool normalize, std::vector<double> mean,
                    std::vector<double> stdv) {
  check_cuda(images, "images");
  TORCH_CHECK(images.dim() == 4 && (images.scalar_type() == at::kByte || images.scalar_type() == at::kFloat),
              "images must be uint8 or fp32 NCHW");
  check_cuda(idx, "idx");
  TORCH_CHECK(idx.scalar_type() == at::kLong && idx.dim() == 1, "idx must be device int64 [B]");
  const int64_t B = idx.numel(), N = images.size(0), C = images.size(1), H = images.size(2), W = images.size(3);
  TORCH_CHECK(box_in.scalar_type() == at::kInt && box_in.dim() == 2 && box_in.size(0) == B && box_in.size(1) == 4 &&
              box_in.is_contiguous(), "box must be contiguous int32 [B, 4] (y0, x0, h, w)");
  const bool* fp = nullptr;
  if (const Tensor* f = opt(flip)) {
    TORCH_CHECK(f->is_cuda() && f->scalar_type() == at::kBool && f->is_contiguous() && f->numel() == B,
                "flip must be device bool [B]");
    fp = f->data_ptr<bool>();
  }
  TORCH_CHECK(out_h >= 1 && out_w >= 1 && out_h <= pdt::img::kMaxSide && out_w <= pdt::img::kMaxSide,
              "resized_crop: output sides must be in [1, ", pdt::img::kMaxSide, "]");
  TORCH_CHECK(out_w % 4 == 0, "resized_crop: output width must be a multiple of 4");
  TORCH_CHECK(N >= 1 && H >= 1 && W >= 1 && H <= pdt::img::kMaxSide && W <= pdt::img::kMaxSide,
              "resized_crop: source sides must be in [1, ", pdt::img::kMaxSide, "] and the source not empty");
  TORCH_CHECK(C >= 1 && C <= 3, "resized_crop: 1 to 3 channels");
  TORCH_CHECK(mean.size() >= (size_t)C && stdv.size() >= (size_t)C, "mean/std per channel");
  TORCH_CHECK(B <= 65535, "resized_crop: at most 65535 samples per call (the grid's z extent)");
  if (!box_in.is_cuda()) check_boxes(box_in, H, W);
  else if (g_sync_check) check_boxes(box_in.cpu(), H, W);
  c10::hip::HIPGuard g(images.get_device());
  const Tensor box = box_in.is_cuda() ? box_in : box_in.to(images.device());
  TORCH_CHECK(box.get_device() == images.get_device() && idx.get_device() == images.get_device(),
              "images, idx and box must be on one device");
  TORCH_CHECK(aligned16(box.data_ptr()), "box must be 16-byte aligned (the kernel loads a row at once)");
  float m[3] = {0.f, 0.f, 0.f}, sd[3] = {1.f, 1.f, 1.f};
  for (int c = 0; c < C; ++c) { m[c] = (float)mean[c]; sd[c] = (float)stdv[c]; }
  auto out = at::empty({B, C, out_h, out_w}, images.options().dtype(at::kFloat));
  pdt::img::launch_resized_crop(images.data_ptr(), images.scalar_type() == at::kByte, N, idx.data_ptr<int64_t>(),
                                box.data_ptr<int32_t>(), fp, out.data_ptr<float>(), (int)B, (int)C, (int)H, (int)W,
                                (int)out_h, (int)out_w, normalize, m, sd, cur_stream(images));
  return out;
}

// every id of a host int32 [B] op tensor names an operation, every row of a host int32 [B, 4] erase
// tensor is a box inside the H x W image (h = 0 or w = 0: no box)
void check_policy(const Tensor& op, const Tensor& erase, int64_t H, int64_t W) {
  const int32_t* o = op.data_ptr<int32_t>();
  const int32_t* p = erase.data_ptr<int32_t>();
  for (int64_t b = 0; b < op.size(0); ++b, p += 4) {
    TORCH_CHECK(o[b] >= 0 && o[b] < pdt::img::kAugOps, "autoaug: op ", b, " = ", o[b], " is not an operation id (0..",
                pdt::img::kAugOps - 1, ")");
    const int64_t y0 = p[0], x0 = p[1], h = p[2], w = p[3];
    TORCH_CHECK(h >= 0 && w >= 0 && y0 >= 0 && x0 >= 0 && y0 + h <= H && x0 + w <= W, "autoaug: erase box ", b,
                " = (y0 ", y0, ", x0 ", x0, ", h ", h, ", w ", w, ") reaches outside the ", H, " x ", W, " image");
  }
}

// x fp32 [B, 3, H, W] in [0, 1]; op int32 [B]; param fp32 [B, 2]; matrix fp32 [B, 6]; erase int32 [B, 4]
// = (y0, x0, h, w): the draws of data/autoaug.py, all on the device of x.  The kernel treats an unknown
// op id as Identity and clamps a box into the image; with PDT_SYNC_CHECK on (every op synchronizes
// anyway) both are copied back and checked instead.  `passes` (1 statistics, 2 apply, 3 both): the loader
// skips the statistics pass when it erases only (every op is Identity), a benchmark times a pass alone.
Tensor autoaug(const Tensor& x, const Tensor& op, const Tensor& param, const Tensor& matrix, const Tensor& erase,
               bool normalize, std::vector<double> mean, std::vector<double> stdv, int64_t passes) {
  check_f32(x, "x");
  TORCH_CHECK(x.dim() == 4 && x.size(1) == 3, "autoaug: x must be fp32 [B, 3, H, W]");
  const int64_t B = x.size(0), H = x.size(2), W = x.size(3);
  TORCH_CHECK(H >= 1 && W >= 1 && H <= pdt::img::kAugMaxSide && W <= pdt::img::kAugMaxSide,
              "autoaug: sides must be in [1, ", pdt::img::kAugMaxSide, "] (the integer statistics are 32-bit)");
  TORCH_CHECK(W % 4 == 0, "autoaug: width must be a multiple of 4");
  TORCH_CHECK(B <= 65535, "autoaug: at most 65535 samples per call (the grid's y extent)");
  check_cuda(op, "op");
  TORCH_CHECK(op.scalar_type() == at::kInt && op.dim() == 1 && op.size(0) == B, "op must be device int32 [B]");
  check_f32(param, "param");
  TORCH_CHECK(param.dim() == 2 && param.size(0) == B && param.size(1) == 2, "param must be device fp32 [B, 2]");
  check_f32(matrix, "matrix");
  TORCH_CHECK(matrix.dim() == 2 && matrix.size(0) == B && matrix.size(1) == 6, "matrix must be device fp32 [B, 6]");
  check_cuda(erase, "erase");
  TORCH_CHECK(erase.scalar_type() == at::kInt && erase.dim() == 2 && erase.size(0) == B && erase.size(1) == 4,
              "erase must be device int32 [B, 4] (y0, x0, h, w)");
  const int dev = x.get_device();
  TORCH_CHECK(op.get_device() == dev && param.get_device() == dev && matrix.get_device() == dev &&
              erase.get_device() == dev, "x, op, param, matrix and erase must be on one device");
  TORCH_CHECK(aligned16(x.data_ptr()) && aligned16(erase.data_ptr()),
              "x and erase must be 16-byte aligned (the kernel loads four pixels and a box at once)");
  TORCH_CHECK(mean.size() >= 3 && stdv.size() >= 3, "mean/std per channel");
  TORCH_CHECK(passes >= 1 && passes <= 3, "autoaug: passes must be 1 (statistics), 2 (apply) or 3 (both)");
  if (g_sync_check) check_policy(op.cpu(), erase.cpu(), H, W);
  c10::hip::HIPGuard g(dev);
  float m[3], sd[3];
  for (int c = 0; c < 3; ++c) { m[c] = (float)mean[c]; sd[c] = (float)stdv[c]; }
  auto out = at::empty_like(x);
  auto ws = at::empty({(int64_t)pdt::img::autoaug_workspace_bytes((int)B)}, x.options().dtype(at::kByte));
  pdt::img::launch_autoaug(x.data_ptr<float>(), op.data_ptr<int32_t>(), param.data_ptr<float>(),
                           matrix.data_ptr<float>(), erase.data_ptr<int32_t>(), out.data_ptr<float>(), ws.data_ptr(),
                           (int)B, (int)H, (int)W, normalize, m, sd, (int)passes, cur_stream(x));
  return out;
}

}  // namespace

PYBIND11_MODULE(_C_img, m) {
  m.doc() = "MI355X (gfx950) input transforms: fused crop + antialiased resize + flip + normalize, and the fused "
            "augmentation policy";
  def_op(m, "resized_crop", &resized_crop, py::arg("images"), py::arg("idx"), py::arg("box"), py::arg("flip"),
         py::arg("out_h"), py::arg("out_w"), py::arg("normalize"), py::arg("mean"), py::arg("std"));
  def_op(m, "autoaug", &autoaug, py::arg("x"), py::arg("op"), py::arg("param"), py::arg("matrix"), py::arg("erase"),
         py::arg("normalize"), py::arg("mean"), py::arg("std"), py::arg("passes") = 3);
  m.def("set_sync_check", [](bool on) { pdt::bind::g_sync_check = on; });
  m.def("sync_check_enabled", []() { return pdt::bind::g_sync_check; });
}
