// Host side of the multicubic value-and-gradient evaluation (cubic_grad.h): which of the two kernels a handle gets, and
// their launchers.  One launch per call whatever the batch size: the binned and column paths have no gradient form.
#include "cubic_grad.h"

namespace interpn {

// The fused kernel runs where the handle keeps the tiled table it gathers from (N = 2, 3; a 4-D handle's tiles are
// left to the runtime-N kernel).
static bool cubic_grad_fused_applies(const GridDesc& g) {
  return g.method == kCubic && g.bricks && !g.cfg.force_generic && (g.ndims == 2 || g.ndims == 3);
}

template <typename T, int N, bool RECT, bool FMA>
static hipError_t cubic_grad_launch_steps(const GridDesc& g, const CubicGradArgs<T, N>& a, size_t lds, unsigned blocks, hipStream_t stream) {
  const int si = g.brick_step[0], sj = g.brick_step[1];
#define GO(SI, SJ) do { g.tag.set("k_cubic_grad", {N, RECT, FMA, SI, SJ}, 0b00110u); hipLaunchKernelGGL((k_cubic_grad<T, N, RECT, FMA, SI, SJ>), dim3(blocks), dim3(kBlock), lds, stream, a); } while (0)
  if (si == 4 && sj == 4) GO(4, 4);
  else if (si == 2 && sj == 4) GO(2, 4);
  else if (si == 2 && sj == 2) GO(2, 2);
  else if (si == 1 && sj == 4) GO(1, 4);
  else if (si == 1 && sj == 1) GO(1, 1);
  else return hipErrorInvalidValue;
#undef GO
  return hipGetLastError();
}

template <typename T, int N>
static hipError_t cubic_grad_launch_fused(const GridDesc& g, const T* const* obs, T* out, T* const* grad, size_t npts,
                                          unsigned long long* first_bad, hipStream_t stream) {
  CubicGradArgs<T, N> a;
  a.bricks = static_cast<const T*>(g.bricks);
  {
    unsigned nb[2];
    size_t bytes = 0;
    cubic_tile_geometry(g, g.brick_step[0], g.brick_step[1], nb, &bytes);
    a.table_bytes = (unsigned)bytes;  // < 4 GiB by construction (maybe_build_cubic_tiles)
  }
  a.out = out;
  a.first_bad = first_bad;
  a.npts = npts;
  a.linearize = g.linearize;
  for (int d = 0; d < N; ++d) {
    a.obs[d] = obs[d];
    a.grad[d] = grad[d];
    a.start[d] = (T)g.start[d];
    a.step[d] = (T)g.step[d];
    a.n[d] = g.n[d];
    a.plane_stride[d] = 0;
  }
  a.nbj = g.brick_nb[1];
  if (N == 3) a.plane_stride[2] = g.brick_nb[0] * g.brick_nb[1] * 16u;  // table[k][bi][bj][16]
  const bool dma = g.brick_step[0] == 1 && g.brick_step[1] == 1;  // cubic_brick.h::cubic_dma
  size_t lds = dma ? (size_t)(kBlock / 64) * cubic_dma_image<T>() : (size_t)kBlock * kCubRow * (sizeof(T) > 4 ? sizeof(T) : 4);
  a.ax.use_lds = 0;
  a.ax.image = nullptr;
  a.ax.image_bytes = 0;
  if (g.kind == kRectilinear) lds += fill_axis_args<T, N>(g, a.ax);
  const unsigned blocks = grid_blocks(npts, 1, g.cfg);
  if (g.kind == kRegular)
    return g.fma ? cubic_grad_launch_steps<T, N, false, true>(g, a, lds, blocks, stream)
                 : cubic_grad_launch_steps<T, N, false, false>(g, a, lds, blocks, stream);
  return g.fma ? cubic_grad_launch_steps<T, N, true, true>(g, a, lds, blocks, stream)
               : cubic_grad_launch_steps<T, N, true, false>(g, a, lds, blocks, stream);
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
