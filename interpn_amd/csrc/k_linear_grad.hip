// Host side of the multilinear value-and-gradient evaluation (linear_grad.h): which of the two kernels a handle gets,
// and their launchers.  One launch per call whatever the batch size: the sweep kernels have no gradient form.
#include <cstdlib>

#include "linear_grad.h"

namespace interpn {

// The fused kernel runs where the handle keeps the table it gathers from: the 2-D bricks, or 3-D bricks of any of the
// layouts 11 / 12 / 22 / f32 2 x 4 x 4.  (3-D handles never have the 4-D cell bricks.)
static bool grad_fused_applies(const GridDesc& g) {
  if (g.method != kLinear || !g.bricks || g.cfg.force_generic) return false;
  if (g.ndims == 2) return true;
  return g.ndims == 3 && g.brick_cell != 1;
}

template <typename T, int N, bool RECT, bool FMA, int PPL, int AXR>
static hipError_t grad_launch_steps(const GridDesc& g, const GradArgs<T, N>& a, size_t lds, unsigned blocks, hipStream_t stream) {
#define GRAD_GO(SI, SJ, CELL)                                                                                          \
  do {                                                                                                                 \
    g.tag.set("k_linear_grad", {N, RECT, FMA, SI, SJ, PPL, AXR, CELL}, 0b00000110u);                                   \
    hipLaunchKernelGGL((k_linear_grad<T, N, RECT, FMA, SI, SJ, PPL, AXR, CELL>), dim3(blocks), dim3(kBlock), lds, stream, a); \
    return hipGetLastError();                                                                                          \
  } while (0)
  if constexpr (N == 2) {
    GRAD_GO(1, 1, 0);
  } else {
    if constexpr (sizeof(T) == 4) {
      if (g.brick_cell == 2) GRAD_GO(1, 1, 2);
    }
    const int si = g.brick_step[0], sj = g.brick_step[1];
    if (si == 1 && sj == 1) GRAD_GO(1, 1, 0);
    if (si == 1 && sj == 2) GRAD_GO(1, 2, 0);
    GRAD_GO(2, 2, 0);
  }
#undef GRAD_GO
}

template <typename T, int N, int PPL>
static hipError_t grad_launch_kind(const GridDesc& g, GradArgs<T, N>& a, size_t lds, size_t axis_lds, size_t npts, hipStream_t stream) {
  const int axr = lane_axes_mode(g);  // axes in lanes (lane_axes.h) or 0 = LDS / L2 search
  a.iters = brick_iters(g, npts, PPL, /*setup=*/g.kind != kRectilinear ? 0 : (axr == 0 ? 2 : 1));
  const size_t nslots = (npts + PPL - 1) / PPL;
  const size_t per_block = (size_t)kBlock * a.iters;
  const unsigned blocks = (unsigned)((nslots + per_block - 1) / per_block);
  if (g.kind == kRegular)
    return g.fma ? grad_launch_steps<T, N, false, true, PPL, 0>(g, a, lds, blocks, stream)
                 : grad_launch_steps<T, N, false, false, PPL, 0>(g, a, lds, blocks, stream);
  if (axr == 2)
    return g.fma ? grad_launch_steps<T, N, true, true, PPL, 2>(g, a, lds, blocks, stream)
                 : grad_launch_steps<T, N, true, false, PPL, 2>(g, a, lds, blocks, stream);
  if (axr == 3)
    return g.fma ? grad_launch_steps<T, N, true, true, PPL, 3>(g, a, lds, blocks, stream)
                 : grad_launch_steps<T, N, true, false, PPL, 3>(g, a, lds, blocks, stream);
  if (axr == 1)
    return g.fma ? grad_launch_steps<T, N, true, true, PPL, 1>(g, a, lds, blocks, stream)
                 : grad_launch_steps<T, N, true, false, PPL, 1>(g, a, lds, blocks, stream);
  return g.fma ? grad_launch_steps<T, N, true, true, PPL, 0>(g, a, lds + axis_lds, blocks, stream)
               : grad_launch_steps<T, N, true, false, PPL, 0>(g, a, lds + axis_lds, blocks, stream);
}

template <typename T, int N>
static hipError_t grad_launch_fused(const GridDesc& g, const T* const* obs, T* out, T* const* grad, size_t npts,
                                    unsigned long long* first_bad, hipStream_t stream) {
  typedef typename LeafVec<T, 2>::type P;
  GradArgs<T, N> a;
  a.bricks = static_cast<const T*>(g.bricks);
  a.out = out;
  a.first_bad = first_bad;
  a.npts = npts;
  for (int d = 0; d < N; ++d) {
    a.obs[d] = obs[d];
    a.grad[d] = grad[d];
    a.start[d] = (T)g.start[d];
    a.step[d] = (T)g.step[d];
    a.n[d] = g.n[d];
  }
  a.nbj = g.brick_nb[1];
  a.nbk = N == 3 ? g.brick_nb[2] : 1u;
  const size_t lds = N == 3 ? (size_t)kBlock * kPieceRow * sizeof(P) + (size_t)kBlock * 16 : 0;
  a.ax.use_lds = 0;
  a.ax.image = nullptr;
  a.ax.image_bytes = 0;
  size_t axis_lds = 0;
  // the 2-D kernel has no other LDS use: its axis image may take the wide budget, as in k_linear2_brick
  if (g.kind == kRectilinear) axis_lds = fill_axis_args<T, N>(g, a.ax, /*big_lds=*/N == 2, /*records=*/true);
  // two points per lane (vector coordinate / result accesses) when every stream is aligned to 2 * sizeof(T); the handle's
  // `ppl` option = 1 forces the scalar form, as for the value kernels
  bool aligned = (reinterpret_cast<uintptr_t>(out) % (2 * sizeof(T))) == 0;
  for (int d = 0; d < N; ++d)
    aligned = aligned && (reinterpret_cast<uintptr_t>(obs[d]) % (2 * sizeof(T))) == 0 &&
              (reinterpret_cast<uintptr_t>(grad[d]) % (2 * sizeof(T))) == 0;
  if (aligned && g.cfg.ppl != 1) return grad_launch_kind<T, N, 2>(g, a, lds, axis_lds, npts, stream);
  return grad_launch_kind<T, N, 1>(g, a, lds, axis_lds, npts, stream);
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
  if (grad_fused_applies(g)) {
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
