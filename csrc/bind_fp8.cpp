// Bindings of the FP8 forward path (csrc/kernels/gemm_fp8.hip, csrc/include/pde_fp8.h).  e4m3 tensors travel as
// uint8 views.
#include <vector>

#include "pde_bind.h"
#include "pde_fp8.h"

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

}  // namespace

void register_fp8(pybind11::module& m) {
  namespace py = pybind11;
  m.def("fp8_quantize", &fp8_quantize);
  m.def("fp8_quantize_many", &fp8_quantize_many);
  m.def("gemm_fp8", &gemm_fp8, py::arg("xq"), py::arg("wq"), py::arg("xs"), py::arg("ws"), py::arg("y"),
        py::arg("bias") = py::none(), py::arg("y2") = py::none());
  m.def("gemm_fp8_tile", []() {
    int bm = 0, bn = 0;
    pde_gemm_fp8_tile(&bm, &bn);
    return std::vector<int64_t>{bm, bn};
  });
}

}  // namespace pde
