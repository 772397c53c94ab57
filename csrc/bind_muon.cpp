// Bindings of Muon's kernels (csrc/kernels/muon.hip, csrc/include/pde_muon.h): the grouped symmetric / rectangular
// GEMM stages, the whole Newton-Schulz iteration, and the prologue / apply streaming kernels.  Lists are one matrix
// per entry; dimension limits are checked here (ValueError) and again by the launchers.
#include <cmath>
#include <vector>

#include "pde_bind.h"
#include "pde_muon.h"

namespace pde {
namespace {

using TList = std::vector<at::Tensor>;
using OptList = std::optional<TList>;

void check_dims(int64_t r, int64_t c, const char* what) {
  if (r < 64 || c < 64 || r % 64 || c % 64 || r * c * 2 >= (1LL << 31)) {
    PyErr_Format(PyExc_ValueError, "%s: matrix dimensions must be multiples of 64 and the matrix below 2 GiB (got %lld x %lld)",
                 what, (long long)r, (long long)c);
    throw pybind11::error_already_set();
  }
}

const at::Tensor& mat(const at::Tensor& t, const char* name, at::ScalarType dt, int64_t r, int64_t c,
                      const at::Tensor& like) {
  check_cuda(t, name, dt, 1);
  TORCH_CHECK(t.dim() == 2 && t.size(0) == r && t.size(1) == c, name, " must be [", r, ", ", c, "], got ", t.sizes());
  TORCH_CHECK(t.device() == like.device(), name, " is on ", t.device(), ", expected ", like.device());
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name, " must be 16-byte aligned");
  return t;
}

std::vector<PdeMuonGemm> sym_table(const TList& p, const OptList& c, const TList& d) {
  const size_t n = p.size();
  TORCH_CHECK(n >= 1 && d.size() == n && (!c.has_value() || c->size() == n), "muon_gemm_sym: lists differ in length");
  std::vector<PdeMuonGemm> tab(n);
  for (size_t i = 0; i < n; ++i) {
    TORCH_CHECK(p[i].dim() == 2, "muon_gemm_sym: 2-D matrices expected");
    const int64_t r = p[i].size(0), k = p[i].size(1);
    check_dims(r, k, "muon_gemm_sym");
    mat(p[i], "p", BF16, r, k, p[0]);
    mat(d[i], "d", BF16, r, r, p[0]);
    const void* cp = c.has_value() ? mat((*c)[i], "c", BF16, r, r, p[0]).data_ptr() : nullptr;
    TORCH_CHECK(d[i].data_ptr() != p[i].data_ptr() && d[i].data_ptr() != cp, "muon_gemm_sym: d aliases an input");
    tab[i] = PdeMuonGemm{p[i].data_ptr(), nullptr, cp, d[i].data_ptr(), (int)r, (int)r, (int)k, 0};
  }
  return tab;
}

std::vector<PdeMuonGemm> rect_table(const TList& a, const TList& b, const TList& c, const TList& d) {
  const size_t n = a.size();
  TORCH_CHECK(n >= 1 && b.size() == n && c.size() == n && d.size() == n, "muon_gemm_rect: lists differ in length");
  std::vector<PdeMuonGemm> tab(n);
  for (size_t i = 0; i < n; ++i) {
    TORCH_CHECK(a[i].dim() == 2 && b[i].dim() == 2, "muon_gemm_rect: 2-D matrices expected");
    const int64_t k = a[i].size(0), r = a[i].size(1), cols = b[i].size(1);
    check_dims(k, r, "muon_gemm_rect");
    check_dims(k, cols, "muon_gemm_rect");
    mat(a[i], "a", BF16, k, r, a[0]);
    mat(b[i], "b", BF16, k, cols, a[0]);
    mat(c[i], "c", BF16, r, cols, a[0]);
    mat(d[i], "d", BF16, r, cols, a[0]);
    TORCH_CHECK(d[i].data_ptr() != a[i].data_ptr() && d[i].data_ptr() != b[i].data_ptr() &&
                    d[i].data_ptr() != c[i].data_ptr(), "muon_gemm_rect: d aliases an input");
    tab[i] = PdeMuonGemm{a[i].data_ptr(), b[i].data_ptr(), c[i].data_ptr(), d[i].data_ptr(), (int)r, (int)cols, (int)k, 0};
  }
  return tab;
}

// d[i] [n, n] = alpha c[i] + beta p[i] p[i]^T (c absent: beta p p^T)
void muon_gemm_sym(const TList& p, const OptList& c, const TList& d, double alpha, double beta) {
  auto tab = sym_table(p, c, d);
  hip_check(pde_muon_gemm_sym(tab.data(), (int)tab.size(), (float)alpha, (float)beta, cur_stream()), "muon_gemm_sym");
}

// d[i] [n, m] = alpha c[i] + beta a[i]^T b[i], a[i] [k, n] (symmetric in Muon's use), b[i] [k, m]
void muon_gemm_rect(const TList& a, const TList& b, const TList& c, const TList& d, double alpha, double beta) {
  auto tab = rect_table(a, b, c, d);
  hip_check(pde_muon_gemm_rect(tab.data(), (int)tab.size(), (float)alpha, (float)beta, cur_stream()), "muon_gemm_rect");
}

// `steps` Newton-Schulz iterations on the wide matrices x[i] [n, m]: 3 launches each.  A and B are [n, n] scratch,
// xalt the ping-pong twin of x; returns true when the result is in xalt (odd steps).
bool muon_ns(const TList& x, const TList& xalt, const TList& A, const TList& B, int64_t steps, double ca, double cb,
             double cc) {
  TORCH_CHECK(steps >= 0 && steps <= 64, "muon_ns: steps out of range");
  for (const auto& t : x) TORCH_CHECK(t.dim() == 2 && t.size(0) <= t.size(1), "muon_ns: x must be wide [n, m], n <= m");
  auto s1a = sym_table(x, std::nullopt, A), s1b = sym_table(xalt, std::nullopt, A);
  auto s2 = sym_table(A, A, B);
  auto s3a = rect_table(B, x, x, xalt), s3b = rect_table(B, xalt, xalt, x);
  const int n = (int)x.size();
  hipStream_t st = cur_stream();
  for (int64_t it = 0; it < steps; ++it) {
    const bool odd = it & 1;
    hip_check(pde_muon_gemm_sym((odd ? s1b : s1a).data(), n, 0.f, 1.f, st), "muon_ns (X X^T)");
    hip_check(pde_muon_gemm_sym(s2.data(), n, (float)cb, (float)cc, st), "muon_ns (b A + c A A)");
    hip_check(pde_muon_gemm_rect((odd ? s3b : s3a).data(), n, (float)ca, 1.f, st), "muon_ns (a X + B X)");
  }
  return steps & 1;
}

std::vector<PdeMuonMat> mat_table(const TList& shaped, const TList& src, const OptList& f32, const TList& dst,
                                  at::ScalarType src_dt, const std::vector<double>* wd, const char* what) {
  const size_t n = shaped.size();
  TORCH_CHECK(n >= 1 && src.size() == n && dst.size() == n && (!f32.has_value() || f32->size() == n) &&
                  (wd == nullptr || wd->size() == n), what, ": lists differ in length");
  std::vector<PdeMuonMat> tab(n);
  for (size_t i = 0; i < n; ++i) {
    TORCH_CHECK(shaped[i].dim() == 2, what, ": 2-D matrices expected");
    const int64_t r = shaped[i].size(0), c = shaped[i].size(1);
    check_dims(r, c, what);
    for (const at::Tensor* t : {&src[i], &dst[i]}) {
      check_cuda(*t, "matrix", src_dt, r * c);
      TORCH_CHECK(t->numel() == r * c && t->device() == shaped[0].device() &&
                      reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0,
                  what, ": every tensor of a matrix holds R * C elements on one device, 16-byte aligned");
    }
    float* fp = nullptr;
    if (f32.has_value()) {
      const at::Tensor& f = (*f32)[i];
      check_cuda(f, "fp32 state", F32, r * c);
      TORCH_CHECK(f.numel() == r * c && f.device() == shaped[0].device() &&
                      reinterpret_cast<uintptr_t>(f.data_ptr()) % 16 == 0,
                  what, ": fp32 state must hold R * C elements on the same device, 16-byte aligned");
      fp = ptr<float>(f);
    }
    tab[i] = PdeMuonMat{src[i].data_ptr(), fp, dst[i].data_ptr(), (int)r, (int)c, 0,
                        std::sqrt(std::max(1.f, (float)r / (float)c)), wd ? (float)(*wd)[i] : 0.f};
  }
  return tab;
}

int64_t muon_partials(const TList& mats) {
  int64_t n = 0;
  for (const auto& t : mats) {
    TORCH_CHECK(t.dim() == 2, "muon_partials: 2-D matrices expected");
    n += pde_muon_tiles((int)t.size(0), (int)t.size(1));
  }
  return n;
}

// g[i] [R, C] bf16 (times grad_scale); mom[i] fp32 (absent: U = g); x0[i]: R * C bf16, written in the wide orientation
void muon_prologue(const TList& g, const OptList& mom, const TList& x0, const at::Tensor& partials, double mu,
                   bool nesterov, double grad_scale) {
  auto tab = mat_table(g, g, mom, x0, BF16, nullptr, "muon_prologue");
  check_cuda(partials, "partials", F32, muon_partials(g));
  TORCH_CHECK(partials.device() == g[0].device(), "muon_prologue: partials on another device");
  hip_check(pde_muon_prologue(tab.data(), (int)tab.size(), ptr<float>(partials), (float)mu, nesterov ? 1 : 0,
                              (float)grad_scale, cur_stream()), "muon_prologue");
}

// w[i] [R, C] bf16, x[i] the wide result; master[i] fp32 (absent: w = O)
void muon_apply(const TList& x, const OptList& master, const TList& w, double lr, const std::vector<double>& wd,
                int64_t step, const OptT& step_dev, const OptT& lr_tab) {
  auto tab = mat_table(w, x, master, w, BF16, &wd, "muon_apply");
  const float* sd = optr<float>(step_dev, "step_dev", F32, 1);
  int lr_len = 0;
  const float* lt = lr_table(lr_tab, w[0], &lr_len);
  hip_check(pde_muon_apply(tab.data(), (int)tab.size(), (float)lr, (int)step, sd, lt, lr_len, cur_stream()), "muon_apply");
}

}  // namespace

void register_muon(pybind11::module& m) {
  namespace py = pybind11;
  m.def("muon_gemm_sym", &muon_gemm_sym, py::arg("p"), py::arg("c"), py::arg("d"), py::arg("alpha"), py::arg("beta"));
  m.def("muon_gemm_rect", &muon_gemm_rect, py::arg("a"), py::arg("b"), py::arg("c"), py::arg("d"), py::arg("alpha"),
        py::arg("beta"));
  m.def("muon_ns", &muon_ns, py::arg("x"), py::arg("xalt"), py::arg("A"), py::arg("B"), py::arg("steps"), py::arg("a"),
        py::arg("b"), py::arg("c"));
  m.def("muon_partials", &muon_partials);
  m.def("muon_prologue", &muon_prologue, py::arg("g"), py::arg("mom"), py::arg("x0"), py::arg("partials"), py::arg("mu"),
        py::arg("nesterov"), py::arg("grad_scale"));
  m.def("muon_apply", &muon_apply, py::arg("x"), py::arg("master"), py::arg("w"), py::arg("lr"), py::arg("wd"),
        py::arg("step") = 0, py::arg("step_dev") = py::none(), py::arg("lr_table") = py::none());
}

}  // namespace pde
