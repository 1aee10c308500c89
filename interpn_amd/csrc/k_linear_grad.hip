// Host side of the multilinear value-and-gradient evaluation (linear_grad.h): which of the two kernels a handle gets,
// and their launchers (the fused kernel's through linear_cell_launch.h).  One launch per call whatever the batch size:
// the sweep kernels have no gradient form.
#include <cstdlib>

#include "linear_cell_launch.h"
#include "linear_grad.h"

namespace interpn {

struct GradKernel {
  static constexpr const char* name = "k_linear_grad";
  template <typename T, int N> using Args = GradArgs<T, N>;
  template <typename T, int N, bool RECT, bool FMA, int SI, int SJ, int PPL, int AXR, int CELL>
  static auto kernel() { return &k_linear_grad<T, N, RECT, FMA, SI, SJ, PPL, AXR, CELL>; }
};

template <typename T, int N>
static hipError_t grad_launch_fused(const GridDesc& g, const T* const* obs, T* out, T* const* grad, size_t npts,
                                    unsigned long long* first_bad, hipStream_t stream) {
  GradArgs<T, N> a;
  a.out = out;
  for (int d = 0; d < N; ++d) {
    a.obs[d] = obs[d];
    a.grad[d] = grad[d];
  }
  // every stream moves as vectors: the coordinates, the values and the N components
  bool two = cell_two_points<T>(g, {out});
  for (int d = 0; d < N; ++d) two = two && cell_two_points<T>(g, {obs[d], grad[d]});
  return cell_launch<GradKernel, T, N>(g, a, npts, first_bad, two, stream);
}

template <typename T>
static hipError_t grad_launch_generic(const GridDesc& g, const T* const* obs, T* out, T* const* grad, size_t npts,
                                      unsigned long long* first_bad, hipStream_t stream) {
  GradGenericArgs<T> a;
  a.vals = static_cast<const T*>(g.vals);
  a.out = out;
  a.first_bad = first_bad;
  a.npts = npts;
  a.ndims = g.ndims;
  a.fma_index = g.ndims <= 6;  // multilinear/regular.rs:337 against regular_recursive.rs:310-313 (k_generic.hip)
  unsigned long long acc = 1;
  for (int d = kMaxDims - 1; d >= 0; --d) {
    const bool used = d < g.ndims;
    a.obs[d] = used ? obs[d] : nullptr;
    a.grad[d] = used ? grad[d] : nullptr;
    a.start[d] = used ? (T)g.start[d] : (T)0;
    a.step[d] = used ? (T)g.step[d] : (T)1;
    a.grid[d] = used ? static_cast<const T*>(g.grid[d]) : nullptr;
    a.n[d] = used ? g.n[d] : 0;
    a.stride[d] = used ? acc : 0;
    if (used) acc *= (unsigned long long)g.n[d];
  }
  const unsigned blocks = grid_blocks(npts, 1, g.cfg);
#define GRAD_GEN(KIND, FMA)                                                                               \
  do {                                                                                                    \
    g.tag.set("k_linear_grad_n", {KIND, FMA}, 0b10u);                                                     \
    hipLaunchKernelGGL((k_linear_grad_n<T, KIND, FMA>), dim3(blocks), dim3(kBlock), 0, stream, a);        \
  } while (0)
  if (g.kind == kRegular) { if (g.fma) GRAD_GEN(kRegular, true); else GRAD_GEN(kRegular, false); }
  else { if (g.fma) GRAD_GEN(kRectilinear, true); else GRAD_GEN(kRectilinear, false); }
#undef GRAD_GEN
  return hipGetLastError();
}

template <typename T>
static hipError_t grad_launch_t(const GridDesc& g, const void* const* obs, void* out, void* const* grad, size_t npts,
                                unsigned long long* first_bad, hipStream_t stream) {
  const T* const* o = reinterpret_cast<const T* const*>(obs);
  T* const* gr = reinterpret_cast<T* const*>(grad);
  if (linear_cell_applies(g)) {
    if (g.ndims == 2) return grad_launch_fused<T, 2>(g, o, static_cast<T*>(out), gr, npts, first_bad, stream);
    return grad_launch_fused<T, 3>(g, o, static_cast<T*>(out), gr, npts, first_bad, stream);
  }
  return grad_launch_generic<T>(g, o, static_cast<T*>(out), gr, npts, first_bad, stream);
}

hipError_t launch_linear_grad(const GridDesc& g, const void* const* obs, void* out, void* const* grad, size_t npts,
                              unsigned long long* first_bad, hipStream_t stream) {
  if (g.method != kLinear || g.ndims < 1 || g.ndims > kMaxDims) return hipErrorInvalidValue;
  if (npts == 0) return hipSuccess;
  if (g.dtype == kF64) return grad_launch_t<double>(g, obs, out, grad, npts, first_bad, stream);
  return grad_launch_t<float>(g, obs, out, grad, npts, first_bad, stream);
}

}  // namespace interpn
