// Shared helpers of the torch-facing binding layer (csrc/ops_bindings.cpp, csrc/bind_*.cpp).
#pragma once
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <optional>

namespace pde {

using OptT = std::optional<at::Tensor>;

inline hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

inline void check_cuda(const at::Tensor& t, const char* name, at::ScalarType dt, int64_t min_numel = 0) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == dt, name, " has dtype ", t.scalar_type(), ", expected ", dt);
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.numel() >= min_numel, name, " has ", t.numel(), " elements, needs >= ", min_numel);
}

template <typename T>
inline T* ptr(const at::Tensor& t) { return reinterpret_cast<T*>(t.data_ptr()); }

template <typename T>
inline T* optr(const OptT& t, const char* name, at::ScalarType dt, int64_t min_numel = 0) {
  if (!t.has_value() || !t->defined()) return nullptr;
  check_cuda(*t, name, dt, min_numel);
  return ptr<T>(*t);
}

// Optional learning-rate table of the optimizer kernels (pde_lr.h): fp32, at least one entry, on the
// parameters' device.  Returns null (and *len = 0) when no table is given.
inline const float* lr_table(const OptT& t, const at::Tensor& params, int* len) {
  *len = 0;
  if (!t.has_value() || !t->defined()) return nullptr;
  TORCH_CHECK(t->scalar_type() == at::kFloat, "lr_table has dtype ", t->scalar_type(), ", expected float32");
  TORCH_CHECK(t->device() == params.device(), "lr_table is on ", t->device(), ", the parameters are on ",
              params.device());
  TORCH_CHECK(t->dim() == 1 && t->is_contiguous(), "lr_table must be a contiguous 1-D tensor");
  TORCH_CHECK(t->numel() >= 1, "lr_table is empty: it needs at least one learning rate");
  TORCH_CHECK(t->numel() <= INT32_MAX, "lr_table has too many entries");
  *len = (int)t->numel();
  return ptr<float>(*t);
}

inline void hip_check(hipError_t e, const char* what) {
  TORCH_CHECK(e == hipSuccess, what, " failed: ", hipGetErrorString(e));
}

constexpr auto F32 = at::kFloat;
constexpr auto BF16 = at::kBFloat16;
constexpr auto I32 = at::kInt;
constexpr auto I64 = at::kLong;
constexpr auto U8 = at::kByte;
constexpr auto F64 = at::kDouble;

// registration hooks of the extra binding units (called from PYBIND11_MODULE in ops_bindings.cpp)
void register_transformer(pybind11::module& m);
void register_resnet(pybind11::module& m);
void register_decode(pybind11::module& m);

}  // namespace pde
