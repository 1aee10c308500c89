// Host side of the point-major evaluation (linear_points.h): whether the fused kernel takes a handle, its launcher
// (through linear_cell_launch.h), and the launchers of the split path's kernels.
#include <cstdlib>

#include "linear_cell_launch.h"
#include "linear_points.h"

namespace interpn {

bool points_fused_applies(const GridDesc& g) { return linear_cell_applies(g); }

struct PointsKernel {
  static constexpr const char* name = "k_linear_points";
  template <typename T, int N> using Args = PointsArgs<T, N>;
  template <typename T, int N, bool RECT, bool FMA, int SI, int SJ, int PPL, int AXR, int CELL>
  static auto kernel() { return &k_linear_points<T, N, RECT, FMA, SI, SJ, PPL, AXR, CELL>; }
};

template <typename T, int N>
static hipError_t points_launch_fused(const GridDesc& g, const T* pts, size_t stride, T* out, size_t npts,
                                      unsigned long long* first_bad, hipStream_t stream) {
  PointsArgs<T, N> a;
  a.pts = pts;
  a.stride = stride;
  a.out = out;
  const bool two = cell_two_points<T>(g, {out});  // one vector store of the results
  a.load = points_load_form<T, N>(g, pts, stride, two);
  return cell_launch<PointsKernel, T, N>(g, a, npts, first_bad, two, stream);
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
