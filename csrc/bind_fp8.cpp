// Bindings of the FP8 forward paths: per-tensor scaling (csrc/kernels/gemm_fp8.hip, csrc/include/pde_fp8.h) and MX
// block scaling (csrc/kernels/gemm_mxfp8.hip, csrc/include/pde_mxfp8.h).  e4m3 tensors travel as uint8 views.
#include <vector>

#include "pde_bind.h"
#include "pde_fp8.h"
#include "pde_mxfp8.h"

namespace pde {
namespace {

bool aligned16(const at::Tensor& t) { return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0; }

void check_scale(const at::Tensor& s, const char* name, const at::Tensor& like) {
  check_cuda(s, name, F32, 2);
  TORCH_CHECK(s.numel() == 2, name, " must be the two-element scale block {s, 1/s}");
  TORCH_CHECK(s.device() == like.device(), name, " is on ", s.device(), ", the data on ", like.device());
}

// src[i] (bf16, numel % 16 == 0) -> dst[i] (uint8, same numel), scales[i] = {s, 1/s}; work: 2 * count zeroed int32
// words on the same device, re-armed by the kernels
void fp8_quantize_many(const std::vector<at::Tensor>& src, const std::vector<at::Tensor>& dst,
                       const std::vector<at::Tensor>& scales, const at::Tensor& work) {
  const size_t n = src.size();
  TORCH_CHECK(n >= 1, "fp8_quantize: no tensors");
  TORCH_CHECK(dst.size() == n && scales.size() == n, "fp8_quantize: src, dst and scales differ in length");
  check_cuda(work, "work", I32, 2 * (int64_t)n);
  std::vector<PdeFp8Tensor> tab(n);
  for (size_t i = 0; i < n; ++i) {
    check_cuda(src[i], "src", BF16, 16);
    check_cuda(dst[i], "dst", U8, 16);
    check_scale(scales[i], "scale", src[i]);
    TORCH_CHECK(src[i].numel() % 16 == 0, "fp8_quantize: the element count must be a multiple of 16");
    TORCH_CHECK(dst[i].numel() == src[i].numel(), "fp8_quantize: dst holds ", dst[i].numel(), " bytes for ",
                src[i].numel(), " values");
    TORCH_CHECK(src[i].device() == work.device() && dst[i].device() == work.device(),
                "fp8_quantize: tensors on different devices");
    TORCH_CHECK(aligned16(src[i]) && aligned16(dst[i]), "fp8_quantize: src and dst must be 16-byte aligned");
    tab[i] = PdeFp8Tensor{src[i].data_ptr(), dst[i].data_ptr(), ptr<float>(scales[i]), src[i].numel()};
  }
  hip_check(pde_fp8_quantize(tab.data(), (int)n, reinterpret_cast<uint32_t*>(work.data_ptr()), cur_stream()),
            "fp8_quantize");
}

void fp8_quantize(const at::Tensor& src, const at::Tensor& dst, const at::Tensor& scale, const at::Tensor& work) {
  fp8_quantize_many({src}, {dst}, {scale}, work);
}

// y [M, N] bf16 = xq [M, K] . wq [N, K]^T / (sx sw) + bias; with y2: y = gelu(pre), y2 = gelu'(pre)
void gemm_fp8(const at::Tensor& xq, const at::Tensor& wq, const at::Tensor& xs, const at::Tensor& ws,
              const at::Tensor& y, const OptT& bias, const OptT& y2) {
  check_cuda(xq, "xq", U8, 1);
  check_cuda(wq, "wq", U8, 1);
  TORCH_CHECK(xq.dim() == 2 && wq.dim() == 2 && xq.size(1) == wq.size(1), "gemm_fp8: xq [M, K] and wq [N, K]");
  const int64_t M = xq.size(0), K = xq.size(1), N = wq.size(0);
  TORCH_CHECK(N % 8 == 0 && K % 64 == 0, "gemm_fp8: needs N % 8 == 0 and K % 64 == 0 (got N ", N, ", K ", K, ")");
  TORCH_CHECK((M + 256) * K < (1LL << 31) && (N + 256) * K < (1LL << 31), "gemm_fp8: operand too large");
  check_scale(xs, "xs", xq);
  check_scale(ws, "ws", xq);
  check_cuda(y, "y", BF16, M * N);
  TORCH_CHECK(y.dim() == 2 && y.size(0) == M && y.size(1) == N, "gemm_fp8: y must be [M, N]");
  TORCH_CHECK(wq.device() == xq.device() && y.device() == xq.device(), "gemm_fp8: tensors on different devices");
  const void* bp = optr<void>(bias, "bias", BF16, N);
  void* y2p = optr<void>(y2, "y2", BF16, M * N);
  TORCH_CHECK(bp == nullptr || (bias->numel() == N && bias->device() == xq.device()), "gemm_fp8: bias must be [N]");
  TORCH_CHECK(y2p == nullptr || (y2->numel() == M * N && y2->device() == xq.device()), "gemm_fp8: y2 must be [M, N]");
  TORCH_CHECK(aligned16(xq) && aligned16(wq) && aligned16(y) && (y2p == nullptr || aligned16(*y2)) &&
                  (bp == nullptr || reinterpret_cast<uintptr_t>(bp) % 8 == 0),
              "gemm_fp8: operands must be 16-byte aligned (bias 8-byte)");
  hip_check(pde_gemm_fp8(xq.data_ptr(), wq.data_ptr(), ptr<float>(xs), ptr<float>(ws), y.data_ptr(), y2p, bp, (int)M,
                         (int)N, (int)K, cur_stream()),
            "gemm_fp8");
}

// src[i] (bf16, numel % 32 == 0) -> dst[i] (uint8, same numel) and scales[i] (uint8, numel / 32): one launch
void mx_quantize_many(const std::vector<at::Tensor>& src, const std::vector<at::Tensor>& dst,
                      const std::vector<at::Tensor>& scales) {
  const size_t n = src.size();
  TORCH_CHECK(n >= 1, "mx_quantize: no tensors");
  TORCH_CHECK(dst.size() == n && scales.size() == n, "mx_quantize: src, dst and scales differ in length");
  std::vector<PdeMxTensor> tab(n);
  for (size_t i = 0; i < n; ++i) {
    check_cuda(src[i], "src", BF16, 32);
    check_cuda(dst[i], "dst", U8, 32);
    check_cuda(scales[i], "scale", U8, 1);
    TORCH_CHECK(src[i].numel() % 32 == 0, "mx_quantize: the element count must be a multiple of 32");
    TORCH_CHECK(dst[i].numel() == src[i].numel() && scales[i].numel() == src[i].numel() / 32, "mx_quantize: dst holds ",
                dst[i].numel(), " bytes and scale ", scales[i].numel(), " for ", src[i].numel(), " values");
    TORCH_CHECK(dst[i].device() == src[0].device() && scales[i].device() == src[0].device() &&
                    src[i].device() == src[0].device(),
                "mx_quantize: tensors on different devices");
    TORCH_CHECK(aligned16(src[i]) && reinterpret_cast<uintptr_t>(dst[i].data_ptr()) % 8 == 0,
                "mx_quantize: src must be 16-byte and dst 8-byte aligned");
    tab[i] = PdeMxTensor{src[i].data_ptr(), dst[i].data_ptr(), ptr<uint8_t>(scales[i]), src[i].numel()};
  }
  hip_check(pde_mx_quantize(tab.data(), (int)n, cur_stream()), "mx_quantize");
}

// y [M, N] bf16 = block-scaled (xq [M, K], xe [M, K / 32]) . (wq [N, K], we [N, K / 32])^T + bias; with y2:
// y = gelu(pre), y2 = gelu'(pre); with aq / ae as well: y again as an MX tensor
void gemm_mxfp8(const at::Tensor& xq, const at::Tensor& wq, const at::Tensor& xe, const at::Tensor& we,
                const at::Tensor& y, const OptT& bias, const OptT& y2, const OptT& aq, const OptT& ae) {
  check_cuda(xq, "xq", U8, 1);
  check_cuda(wq, "wq", U8, 1);
  TORCH_CHECK(xq.dim() == 2 && wq.dim() == 2 && xq.size(1) == wq.size(1), "gemm_mxfp8: xq [M, K] and wq [N, K]");
  const int64_t M = xq.size(0), K = xq.size(1), N = wq.size(0);
  TORCH_CHECK(N % 8 == 0 && K % 128 == 0, "gemm_mxfp8: needs N % 8 == 0 and K % 128 == 0 (got N ", N, ", K ", K, ")");
  TORCH_CHECK((M + 256) * K < (1LL << 31) && (N + 256) * K < (1LL << 31), "gemm_mxfp8: operand too large");
  check_cuda(xe, "xe", U8, M * K / 32);
  check_cuda(we, "we", U8, N * K / 32);
  TORCH_CHECK(xe.numel() == M * K / 32 && we.numel() == N * K / 32, "gemm_mxfp8: scales must be [rows, K / 32]");
  check_cuda(y, "y", BF16, M * N);
  TORCH_CHECK(y.dim() == 2 && y.size(0) == M && y.size(1) == N, "gemm_mxfp8: y must be [M, N]");
  const void* bp = optr<void>(bias, "bias", BF16, N);
  void* y2p = optr<void>(y2, "y2", BF16, M * N);
  void* aqp = optr<void>(aq, "aq", U8, M * N);
  void* aep = optr<void>(ae, "ae", U8, M * N / 32);
  TORCH_CHECK((aqp == nullptr) == (aep == nullptr) && (aqp == nullptr || (y2p != nullptr && N % 32 == 0)),
              "gemm_mxfp8: aq and ae go together, with y2 and N % 32 == 0");
  TORCH_CHECK(bp == nullptr || bias->numel() == N, "gemm_mxfp8: bias must be [N]");
  TORCH_CHECK((y2p == nullptr || y2->numel() == M * N) && (aqp == nullptr || (aq->numel() == M * N && ae->numel() == M * N / 32)),
              "gemm_mxfp8: y2 and aq must be [M, N], ae [M, N / 32]");
  for (const at::Tensor* t : {&wq, &xe, &we, &y, bp ? &*bias : &xq, y2p ? &*y2 : &xq, aqp ? &*aq : &xq, aep ? &*ae : &xq})
    TORCH_CHECK(t->device() == xq.device(), "gemm_mxfp8: tensors on different devices");
  TORCH_CHECK(aligned16(xq) && aligned16(wq) && aligned16(y) && (y2p == nullptr || aligned16(*y2)) &&
                  reinterpret_cast<uintptr_t>(xe.data_ptr()) % 4 == 0 && reinterpret_cast<uintptr_t>(we.data_ptr()) % 4 == 0 &&
                  (bp == nullptr || reinterpret_cast<uintptr_t>(bp) % 8 == 0) &&
                  (aqp == nullptr || reinterpret_cast<uintptr_t>(aqp) % 8 == 0),
              "gemm_mxfp8: operands must be 16-byte aligned (scales 4-byte, bias and aq 8-byte)");
  hip_check(pde_gemm_mxfp8(xq.data_ptr(), wq.data_ptr(), xe.data_ptr(), we.data_ptr(), y.data_ptr(), y2p, bp, aqp, aep,
                           (int)M, (int)N, (int)K, cur_stream()),
            "gemm_mxfp8");
}

}  // namespace

void register_fp8(pybind11::module& m) {
  namespace py = pybind11;
  m.def("fp8_quantize", &fp8_quantize);
  m.def("fp8_quantize_many", &fp8_quantize_many);
  m.def("gemm_fp8", &gemm_fp8, py::arg("xq"), py::arg("wq"), py::arg("xs"), py::arg("ws"), py::arg("y"),
        py::arg("bias") = py::none(), py::arg("y2") = py::none());
  m.def("mx_quantize_many", &mx_quantize_many);
  m.def("gemm_mxfp8", &gemm_mxfp8, py::arg("xq"), py::arg("wq"), py::arg("xe"), py::arg("we"), py::arg("y"),
        py::arg("bias") = py::none(), py::arg("y2") = py::none(), py::arg("aq") = py::none(), py::arg("ae") = py::none());
  m.def("gemm_fp8_tile", []() {
    int bm = 0, bn = 0;
    pde_gemm_fp8_tile(&bm, &bn);
    return std::vector<int64_t>{bm, bn};
  });
}

}  // namespace pde
