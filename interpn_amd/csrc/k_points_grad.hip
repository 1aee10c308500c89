// Host side of the point-major value-and-gradient evaluation (points_grad.h): whether a fused kernel takes a handle,
// their launchers (the multilinear one through linear_cell_launch.h, the multicubic one through cubic_cell_launch.h:
// each sets its kernel's own arguments), the gradient-row store form, and the launcher of the split path's interleaving
// kernel.
#include <cstdlib>

#include "cubic_cell_launch.h"
#include "linear_cell_launch.h"
#include "points_grad.h"

namespace interpn {

bool points_fused_applies(const GridDesc& g);  // k_linear_points.hip

// Multilinear: where k_linear_points runs (points_fused_applies), rows of up to kPointsGradMaxStride elements.
// Multicubic: where k_cubic_grad runs (cubic_grad_fused_applies), the tiled table of a 2-D or 3-D handle.
bool points_grad_fused_applies(const GridDesc& g, size_t stride, size_t gstride) {
  if (g.method == kLinear) return points_fused_applies(g) && stride <= kPointsGradMaxStride && gstride <= kPointsGradMaxStride;
  return cubic_grad_fused_applies(g);
}

struct PointsGradKernel {
  static constexpr const char* name = "k_linear_points_grad";
  template <typename T, int N> using Args = PointsGradArgs<T, N>;
  template <typename T, int N, bool RECT, bool FMA, int SI, int SJ, int PPL, int AXR, int CELL>
  static auto kernel() { return &k_linear_points_grad<T, N, RECT, FMA, SI, SJ, PPL, AXR, CELL>; }
};

template <typename T, int N>
static hipError_t pg_launch_linear(const GridDesc& g, const T* pts, size_t stride, T* out, T* grad, size_t gstride, size_t npts,
                                   unsigned long long* first_bad, hipStream_t stream) {
  PointsGradArgs<T, N> a;
  a.pts = pts;
  a.stride = stride;
  a.out = out;
  a.grad = grad;
  a.gstride = gstride;
  const bool two = cell_two_points<T>(g, {out});  // one vector store of the values
  a.load = points_load_form<T, N>(g, pts, stride, two);
  // the gradient-row store: packed rows whose base is aligned to two elements take vector stores of the lane's own
  // elements (every lane's first element is then aligned too: PPL * N is even, or the form is not compiled), and in 3-D
  // f64 with two points per lane the wave's span through LDS unless option points_store = 1 keeps the per-lane stores:
  // measured 1.74 against 1.92 ms per 1e8 points behind the LDS load, 2.00 against 2.17 behind the per-lane load (regular
  // 64^3; rectilinear 1.69 / 1.90), level at 1e6 points; element stores cost 4.2 - 5.2 ms there.
  // Anything else, and option points_store = 3: element stores
  a.store = kPointsStoreElem;
  if (gstride == (size_t)N && aligned2<T>(grad)) {
    a.store = kPointsStoreWide;
    if (N == 3 && sizeof(T) == 8 && two && g.cfg.points_store != kPointsStoreWide) a.store = kPointsStoreLds;
  }
  if (g.cfg.points_store == 3) a.store = kPointsStoreElem;
  return cell_launch<PointsGradKernel, T, N>(g, a, npts, first_bad, two, stream);
}

struct CubicPointsGradKernel {
  static constexpr const char* name = "k_cubic_points_grad";
  template <typename T, int N> using Args = CubicPointsGradArgs<T, N>;
  template <typename T, int N, bool RECT, bool FMA, int SI, int SJ>
  static auto kernel() { return &k_cubic_points_grad<T, N, RECT, FMA, SI, SJ>; }
};

template <typename T, int N>
static hipError_t pg_launch_cubic(const GridDesc& g, const T* pts, size_t stride, T* out, T* grad, size_t gstride, size_t npts,
                                  unsigned long long* first_bad, hipStream_t stream) {
  CubicPointsGradArgs<T, N> a;
  a.pts = pts;
  a.stride = stride;
  a.out = out;
  a.grad = grad;
  a.gstride = gstride;
  a.vec2_load = N == 2 && stride == 2 && aligned2<T>(pts);
  a.vec2_store = N == 2 && gstride == 2 && aligned2<T>(grad);
  return cubic_cell_launch<CubicPointsGradKernel, T, N>(g, a, npts, first_bad, grid_blocks(npts, 1, g.cfg), stream);
}

template <typename T>
static hipError_t pg_launch_t(const GridDesc& g, const void* pts, size_t stride, void* out, void* grad, size_t gstride, size_t npts,
                              unsigned long long* first_bad, hipStream_t stream) {
  const T* p = static_cast<const T*>(pts);
  T* o = static_cast<T*>(out);
  T* gr = static_cast<T*>(grad);
  if (g.method == kCubic) {
    if (g.ndims == 2) return pg_launch_cubic<T, 2>(g, p, stride, o, gr, gstride, npts, first_bad, stream);
    return pg_launch_cubic<T, 3>(g, p, stride, o, gr, gstride, npts, first_bad, stream);
  }
  if (g.ndims == 2) return pg_launch_linear<T, 2>(g, p, stride, o, gr, gstride, npts, first_bad, stream);
  return pg_launch_linear<T, 3>(g, p, stride, o, gr, gstride, npts, first_bad, stream);
}

hipError_t launch_points_grad(const GridDesc& g, const void* pts, size_t stride, void* out, void* grad, size_t gstride, size_t npts,
                              unsigned long long* first_bad, hipStream_t stream) {
  if (!points_grad_fused_applies(g, stride, gstride) || stride < (size_t)g.ndims || gstride < (size_t)g.ndims) return hipErrorInvalidValue;
  if (npts == 0) return hipSuccess;
  if (g.dtype == kF64) return pg_launch_t<double>(g, pts, stride, out, grad, gstride, npts, first_bad, stream);
  return pg_launch_t<float>(g, pts, stride, out, grad, gstride, npts, first_bad, stream);
}

template <typename T>
static hipError_t join_launch_t(const GridDesc& g, const void* const* src, void* grad, size_t gstride, size_t count, hipStream_t stream) {
  JoinArgs<T> a;
  a.grad = static_cast<T*>(grad);
  a.gstride = gstride;
  a.count = count;
  a.ndims = g.ndims;
  for (int d = 0; d < kMaxDims; ++d) a.src[d] = d < g.ndims ? static_cast<const T*>(src[d]) : nullptr;
  const size_t blocks = (count + kBlock - 1) / kBlock;
  if (blocks > (1u << 23)) return hipErrorInvalidValue;  // (slices are far smaller)
  hipLaunchKernelGGL((k_join_grad<T>), dim3((unsigned)blocks), dim3(kBlock), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_join_grad(const GridDesc& g, const void* const* src, void* grad, size_t gstride, size_t count, hipStream_t stream) {
  if (g.ndims < 1 || g.ndims > kMaxDims || gstride < (size_t)g.ndims) return hipErrorInvalidValue;
  if (count == 0) return hipSuccess;
  if (g.dtype == kF64) return join_launch_t<double>(g, src, grad, gstride, count, stream);
  return join_launch_t<float>(g, src, grad, gstride, count, stream);
}

}  // namespace interpn
