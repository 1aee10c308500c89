// Host side of the point-major evaluation (linear_points.h): whether the fused kernel takes a handle, its launchers (the
// dispatch of k_linear_grad.hip), the coordinate load form, and the launchers of the split path's kernels.
#include <cstdlib>

#include "linear_points.h"

namespace interpn {

// The fused kernel runs where the handle keeps the table it gathers from: the 2-D bricks, or 3-D bricks of any of the
// layouts 11 / 12 / 22 / f32 2 x 4 x 4.  (3-D handles never have the 4-D cell bricks.)
bool points_fused_applies(const GridDesc& g) {
  if (g.method != kLinear || !g.bricks || g.cfg.force_generic) return false;
  if (g.ndims == 2) return true;
  return g.ndims == 3 && g.brick_cell != 1;
}

template <typename T, int N, bool RECT, bool FMA, int PPL, int AXR>
static hipError_t points_launch_steps(const GridDesc& g, const PointsArgs<T, N>& a, size_t lds, unsigned blocks, hipStream_t stream) {
#define POINTS_GO(SI, SJ, CELL)                                                                                          \
  do {                                                                                                                   \
    g.tag.set("k_linear_points", {N, RECT, FMA, SI, SJ, PPL, AXR, CELL}, 0b00000110u);                                   \
    hipLaunchKernelGGL((k_linear_points<T, N, RECT, FMA, SI, SJ, PPL, AXR, CELL>), dim3(blocks), dim3(kBlock), lds, stream, a); \
    return hipGetLastError();                                                                                            \
  } while (0)
  if constexpr (N == 2) {
    POINTS_GO(1, 1, 0);
  } else {
    if constexpr (sizeof(T) == 4) {
      if (g.brick_cell == 2) POINTS_GO(1, 1, 2);
    }
    const int si = g.brick_step[0], sj = g.brick_step[1];
    if (si == 1 && sj == 1) POINTS_GO(1, 1, 0);
    if (si == 1 && sj == 2) POINTS_GO(1, 2, 0);
    POINTS_GO(2, 2, 0);
  }
#undef POINTS_GO
}

template <typename T, int N, int PPL>
static hipError_t points_launch_kind(const GridDesc& g, PointsArgs<T, N>& a, size_t lds, size_t axis_lds, size_t npts, hipStream_t stream) {
  const int axr = lane_axes_mode(g);  // axes in lanes (lane_axes.h) or 0 = LDS / L2 search
  a.iters = brick_iters(g, npts, PPL, /*setup=*/g.kind != kRectilinear ? 0 : (axr == 0 ? 2 : 1));
  const size_t nslots = (npts + PPL - 1) / PPL;
  const size_t per_block = (size_t)kBlock * a.iters;
  const unsigned blocks = (unsigned)((nslots + per_block - 1) / per_block);
  if (g.kind == kRegular)
    return g.fma ? points_launch_steps<T, N, false, true, PPL, 0>(g, a, lds, blocks, stream)
                 : points_launch_steps<T, N, false, false, PPL, 0>(g, a, lds, blocks, stream);
  if (axr == 2)
    return g.fma ? points_launch_steps<T, N, true, true, PPL, 2>(g, a, lds, blocks, stream)
                 : points_launch_steps<T, N, true, false, PPL, 2>(g, a, lds, blocks, stream);
  if (axr == 3)
    return g.fma ? points_launch_steps<T, N, true, true, PPL, 3>(g, a, lds, blocks, stream)
                 : points_launch_steps<T, N, true, false, PPL, 3>(g, a, lds, blocks, stream);
  if (axr == 1)
    return g.fma ? points_launch_steps<T, N, true, true, PPL, 1>(g, a, lds, blocks, stream)
                 : points_launch_steps<T, N, true, false, PPL, 1>(g, a, lds, blocks, stream);
  return g.fma ? points_launch_steps<T, N, true, true, PPL, 0>(g, a, lds + axis_lds, blocks, stream)
               : points_launch_steps<T, N, true, false, PPL, 0>(g, a, lds + axis_lds, blocks, stream);
}

template <typename T, int N>
static hipError_t points_launch_fused(const GridDesc& g, const T* pts, size_t stride, T* out, size_t npts,
                                      unsigned long long* first_bad, hipStream_t stream) {
  typedef typename LeafVec<T, 2>::type P;
  PointsArgs<T, N> a;
  a.bricks = static_cast<const T*>(g.bricks);
  a.pts = pts;
  a.stride = stride;
  a.out = out;
  a.first_bad = first_bad;
  a.npts = npts;
  for (int d = 0; d < N; ++d) {
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
  // two points per lane (one vector store of the results) when `out` is aligned to 2 * sizeof(T); the handle's `ppl`
  // option = 1 forces the scalar form, as for the value kernels
  const bool two = (reinterpret_cast<uintptr_t>(out) % (2 * sizeof(T))) == 0 && g.cfg.ppl != 1;
  // packed rows whose base is aligned to two elements: vector loads of the lane's own elements (every lane's first element
  // is then aligned too: PPL * N is even, or the form is not compiled); anything else: element loads
  a.load = kPointsLoadElem;
  if (stride == (size_t)N && (reinterpret_cast<uintptr_t>(pts) % (2 * sizeof(T))) == 0) {
    a.load = kPointsLoadWide;
    // 3-D f64 with two points per lane: the wave's span through LDS instead, the faster of the two forms (1.25 against
    // 1.51 ms per 1e8 points on 64^3); option points_load = 1 keeps the per-lane loads
    if (N == 3 && sizeof(T) == 8 && two && g.cfg.points_load != kPointsLoadWide) a.load = kPointsLoadLds;
  }
  if (g.cfg.points_load == 3) a.load = kPointsLoadElem;  // testing / measurements: element loads whatever the layout
  if (two) return points_launch_kind<T, N, 2>(g, a, lds, axis_lds, npts, stream);
  return points_launch_kind<T, N, 1>(g, a, lds, axis_lds, npts, stream);
}

template <typename T>
static hipError_t points_launch_t(const GridDesc& g, const void* pts, size_t stride, void* out, size_t npts,
                                  unsigned long long* first_bad, hipStream_t stream) {
  if (g.ndims == 2) return points_launch_fused<T, 2>(g, static_cast<const T*>(pts), stride, static_cast<T*>(out), npts, first_bad, stream);
  return points_launch_fused<T, 3>(g, static_cast<const T*>(pts), stride, static_cast<T*>(out), npts, first_bad, stream);
}

hipError_t launch_linear_points(const GridDesc& g, const void* pts, size_t stride, void* out, size_t npts,
                                unsigned long long* first_bad, hipStream_t stream) {
  if (!points_fused_applies(g) || stride < (size_t)g.ndims) return hipErrorInvalidValue;
  if (npts == 0) return hipSuccess;
  if (g.dtype == kF64) return points_launch_t<double>(g, pts, stride, out, npts, first_bad, stream);
  return points_launch_t<float>(g, pts, stride, out, npts, first_bad, stream);
}

template <typename T>
static hipError_t split_launch_t(const GridDesc& g, const void* pts, size_t stride, void* const* dst, size_t count, hipStream_t stream) {
  SplitArgs<T> a;
  a.pts = static_cast<const T*>(pts);
  a.stride = stride;
  a.count = count;
  a.ndims = g.ndims;
  for (int d = 0; d < kMaxDims; ++d) a.dst[d] = d < g.ndims ? static_cast<T*>(dst[d]) : nullptr;
  const size_t blocks = (count + kBlock - 1) / kBlock;
  if (blocks > (1u << 23)) return hipErrorInvalidValue;  // (slices are far smaller)
  hipLaunchKernelGGL((k_split_points<T>), dim3((unsigned)blocks), dim3(kBlock), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_split_points(const GridDesc& g, const void* pts, size_t stride, void* const* dst, size_t count, hipStream_t stream) {
  if (g.ndims < 1 || g.ndims > kMaxDims || stride < (size_t)g.ndims) return hipErrorInvalidValue;
  if (count == 0) return hipSuccess;
  if (g.dtype == kF64) return split_launch_t<double>(g, pts, stride, dst, count, stream);
  return split_launch_t<float>(g, pts, stride, dst, count, stream);
}

hipError_t launch_points_bad_begin(unsigned long long* word, unsigned long long* saved, hipStream_t stream) {
  hipLaunchKernelGGL(k_points_bad_begin, dim3(1), dim3(1), 0, stream, word, saved);
  return hipGetLastError();
}

hipError_t launch_points_bad_end(unsigned long long* word, const unsigned long long* saved, unsigned long long begin, hipStream_t stream) {
  hipLaunchKernelGGL(k_points_bad_end, dim3(1), dim3(1), 0, stream, word, saved, begin);
  return hipGetLastError();
}

}  // namespace interpn
