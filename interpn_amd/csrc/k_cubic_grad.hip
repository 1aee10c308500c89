// Host side of the multicubic value-and-gradient evaluation (cubic_grad.h): which of the two kernels a handle gets
// (cubic_grad_fused_applies, cubic_cell_launch.h), the fused kernel's own arguments in front of the shared launcher of
// cubic_cell_launch.h, and the launcher of the runtime-N kernel.  One launch per call whatever the batch size: the binned
// and column paths have no gradient form.
#include "cubic_cell_launch.h"
#include "cubic_grad.h"

namespace interpn {

struct CubicGradKernel {
  static constexpr const char* name = "k_cubic_grad";
  template <typename T, int N> using Args = CubicGradArgs<T, N>;
  template <typename T, int N, bool RECT, bool FMA, int SI, int SJ>
  static auto kernel() { return &k_cubic_grad<T, N, RECT, FMA, SI, SJ>; }
};

template <typename T, int N>
static hipError_t cubic_grad_launch_fused(const GridDesc& g, const T* const* obs, T* out, T* const* grad, size_t npts,
                                          unsigned long long* first_bad, hipStream_t stream) {
  CubicGradArgs<T, N> a;
  a.out = out;
  for (int d = 0; d < N; ++d) {
    a.obs[d] = obs[d];
    a.grad[d] = grad[d];
  }
  return cubic_cell_launch<CubicGradKernel, T, N>(g, a, npts, first_bad, grid_blocks(npts, 1, g.cfg), stream);
}

template <typename T>
static hipError_t cubic_grad_launch_generic(const GridDesc& g, const T* const* obs, T* out, T* const* grad, size_t npts,
                                            unsigned long long* first_bad, hipStream_t stream) {
  CubicGradGenericArgs<T> a;
  a.vals = static_cast<const T*>(g.vals);
  a.out = out;
  a.first_bad = first_bad;
  a.npts = npts;
  a.ndims = g.ndims;
  a.linearize = g.linearize;
  a.fma_linear = g.ndims >= 5;  // the arm of the reference the value path runs (k_generic.hip)
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
    g.tag.set("k_cubic_grad_n", {KIND, FMA}, 0b10u);                                                      \
    hipLaunchKernelGGL((k_cubic_grad_n<T, KIND, FMA>), dim3(blocks), dim3(kBlock), 0, stream, a);         \
  } while (0)
  if (g.kind == kRegular) { if (g.fma) GRAD_GEN(kRegular, true); else GRAD_GEN(kRegular, false); }
  else { if (g.fma) GRAD_GEN(kRectilinear, true); else GRAD_GEN(kRectilinear, false); }
#undef GRAD_GEN
  return hipGetLastError();
}

template <typename T>
static hipError_t cubic_grad_launch_t(const GridDesc& g, const void* const* obs, void* out, void* const* grad, size_t npts,
                                      unsigned long long* first_bad, hipStream_t stream) {
  const T* const* o = reinterpret_cast<const T* const*>(obs);
  T* const* gr = reinterpret_cast<T* const*>(grad);
  if (cubic_grad_fused_applies(g)) {
    if (g.ndims == 2) return cubic_grad_launch_fused<T, 2>(g, o, static_cast<T*>(out), gr, npts, first_bad, stream);
    return cubic_grad_launch_fused<T, 3>(g, o, static_cast<T*>(out), gr, npts, first_bad, stream);
  }
  return cubic_grad_launch_generic<T>(g, o, static_cast<T*>(out), gr, npts, first_bad, stream);
}

hipError_t launch_cubic_grad(const GridDesc& g, const void* const* obs, void* out, void* const* grad, size_t npts,
                             unsigned long long* first_bad, hipStream_t stream) {
  if (g.method != kCubic || g.ndims < 1 || g.ndims > kMaxDims) return hipErrorInvalidValue;
  if (npts == 0) return hipSuccess;
  if (g.dtype == kF64) return cubic_grad_launch_t<double>(g, obs, out, grad, npts, first_bad, stream);
  return cubic_grad_launch_t<float>(g, obs, out, grad, npts, first_bad, stream);
}

}  // namespace interpn
