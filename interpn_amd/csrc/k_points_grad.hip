// Host side of the point-major value-and-gradient evaluation (points_grad.h): whether a fused kernel takes a handle,
// their launchers (the multilinear one through linear_cell_launch.h, the multicubic one with the dispatch of
// k_cubic_grad.hip), the gradient-row store form, and the launcher of the split path's interleaving kernel.
#include <cstdlib>

#include "linear_cell_launch.h"
#include "points_grad.h"

namespace interpn {

bool points_fused_applies(const GridDesc& g);  // k_linear_points.hip

// Multilinear: where k_linear_points runs (points_fused_applies), rows of up to kPointsGradMaxStride elements.
// Multicubic: where k_cubic_grad runs, the tiled table of a 2-D or 3-D handle.
bool points_grad_fused_applies(const GridDesc& g, size_t stride, size_t gstride) {
  if (g.method == kLinear) return points_fused_applies(g) && stride <= kPointsGradMaxStride && gstride <= kPointsGradMaxStride;
  return g.method == kCubic && g.bricks && !g.cfg.force_generic && (g.ndims == 2 || g.ndims == 3);
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

template <typename T, int N, bool RECT, bool FMA>
static hipError_t pg_cubic_steps(const GridDesc& g, const CubicPointsGradArgs<T, N>& a, size_t lds, unsigned blocks, hipStream_t stream) {
  const int si = g.brick_step[0], sj = g.brick_step[1];
#define GO(SI, SJ) do { g.tag.set("k_cubic_points_grad", {N, RECT, FMA, SI, SJ}, 0b00110u); hipLaunchKernelGGL((k_cubic_points_grad<T, N, RECT, FMA, SI, SJ>), dim3(blocks), dim3(kBlock), lds, stream, a); } while (0)
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
static hipError_t pg_launch_cubic(const GridDesc& g, const T* pts, size_t stride, T* out, T* grad, size_t gstride, size_t npts,
                                  unsigned long long* first_bad, hipStream_t stream) {
  CubicPointsGradArgs<T, N> a;
  a.bricks = static_cast<const T*>(g.bricks);
  {
    unsigned nb[2];
    size_t bytes = 0;
    cubic_tile_geometry(g, g.brick_step[0], g.brick_step[1], nb, &bytes);
    a.table_bytes = (unsigned)bytes;  // < 4 GiB by construction (maybe_build_cubic_tiles)
  }
  a.pts = pts;
  a.stride = stride;
  a.out = out;
  a.grad = grad;
  a.gstride = gstride;
  a.first_bad = first_bad;
  a.npts = npts;
  a.linearize = g.linearize;
  a.vec2_load = N == 2 && stride == 2 && aligned2<T>(pts);
  a.vec2_store = N == 2 && gstride == 2 && aligned2<T>(grad);
  for (int d = 0; d < N; ++d) {
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
    return g.fma ? pg_cubic_steps<T, N, false, true>(g, a, lds, blocks, stream)
                 : pg_cubic_steps<T, N, false, false>(g, a, lds, blocks, stream);
  return g.fma ? pg_cubic_steps<T, N, true, true>(g, a, lds, blocks, stream)
               : pg_cubic_steps<T, N, true, false>(g, a, lds, blocks, stream);
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
