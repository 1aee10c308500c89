// Point-major field sets: the launchers of the fused kernel and of the split path's join (linear_fields_points.h).
#include "linear_fields_points.h"

namespace interpn {

template <typename T, int N, bool RECT, bool FMA>
static hipError_t launch_n(const GridDesc& g, const void* table, int nfields, const void* pts, size_t stride, void* out,
                           size_t out_stride, size_t npts, unsigned long long* first_bad, hipStream_t stream) {
  typedef FieldsLayout<T, N> L;
  typedef FieldsPointsLayout<T, N> PL;
  FieldsPointsArgs<T, N> a = {};
  a.table = static_cast<const unsigned char*>(table);
  a.pts = static_cast<const T*>(pts);
  a.stride = stride;
  a.out = static_cast<T*>(out);
  a.out_stride = out_stride;
  a.first_bad = first_bad;
  a.npts = npts;
  a.nfields = nfields;
  // dense rows: the wave's span through LDS (element loads: every element-aligned base is aligned enough)
  a.load = stride == (size_t)N ? kPointsLoadLds : kPointsLoadElem;
  a.groups = (unsigned)((nfields + L::P - 1) / L::P);
  unsigned acc = a.groups;
  for (int d = N - 1; d >= 0; --d) {
    a.start[d] = (T)g.start[d];
    a.step[d] = (T)g.step[d];
    a.n[d] = g.n[d];
    a.cstride[d] = acc;
    acc *= (unsigned)(g.n[d] - 1);
  }
  // LDS: the axis image of a rectilinear grid while it fits Thresholds::axis_lds (rect_args.h), then the waves' areas
  size_t lds = 0;
  if constexpr (RECT) lds = (fill_axis_args<T, N>(g, a.ax, /*big_lds=*/false, /*records=*/true) + 15) & ~(size_t)15;
  lds += (size_t)(kBlock / 64) * PL::kWaveLds;
  g.tag.set("k_linear_fields_points", {N, RECT, FMA}, 0b110u);
  hipLaunchKernelGGL((k_linear_fields_points<T, N, RECT, FMA>), dim3(grid_blocks(npts, 1, g.cfg)), dim3(kBlock), lds, stream, a);
  return hipGetLastError();
}

hipError_t launch_linear_fields_points(const GridDesc& g, const void* table, int nfields, const void* pts, size_t stride, void* out,
                                       size_t out_stride, size_t npts, unsigned long long* first_bad, hipStream_t stream) {
  if (stride < (size_t)g.ndims || nfields < 1 || out_stride < (size_t)nfields) return hipErrorInvalidValue;
  if (npts == 0) return hipSuccess;
#define FIELDS_POINTS_CASE(T, N)                                                                                               \
  if (g.kind == kRectilinear)                                                                                                  \
    return g.fma ? launch_n<T, N, true, true>(g, table, nfields, pts, stride, out, out_stride, npts, first_bad, stream)       \
                 : launch_n<T, N, true, false>(g, table, nfields, pts, stride, out, out_stride, npts, first_bad, stream);     \
  return g.fma ? launch_n<T, N, false, true>(g, table, nfields, pts, stride, out, out_stride, npts, first_bad, stream)        \
               : launch_n<T, N, false, false>(g, table, nfields, pts, stride, out, out_stride, npts, first_bad, stream);
  if (g.ndims == 2) {
    if (g.dtype == kF64) { FIELDS_POINTS_CASE(double, 2) }
    FIELDS_POINTS_CASE(float, 2)
  }
  if (g.ndims == 3) {
    if (g.dtype == kF64) { FIELDS_POINTS_CASE(double, 3) }
    FIELDS_POINTS_CASE(float, 3)
  }
#undef FIELDS_POINTS_CASE
  return hipErrorInvalidValue;
}

template <typename T>
static hipError_t join_t(const void* src, size_t pitch, size_t nfields, void* out, size_t out_stride, size_t count, hipStream_t stream) {
  JoinFieldsArgs<T> a;
  a.src = static_cast<const T*>(src);
  a.pitch = pitch;
  a.out = static_cast<T*>(out);
  a.out_stride = out_stride;
  a.count = count;
  a.nfields = nfields;
  const size_t blocks = (count + kBlock - 1) / kBlock;
  if (blocks > (1u << 23)) return hipErrorInvalidValue;  // (slices are far smaller)
  hipLaunchKernelGGL((k_join_fields<T>), dim3((unsigned)blocks), dim3(kBlock), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_join_fields(const GridDesc& g, const void* src, size_t pitch, size_t nfields, void* out, size_t out_stride,
                              size_t count, hipStream_t stream) {
  if (nfields < 1 || out_stride < nfields || pitch < count) return hipErrorInvalidValue;
  if (count == 0) return hipSuccess;
  if (g.dtype == kF64) return join_t<double>(src, pitch, nfields, out, out_stride, count, stream);
  return join_t<float>(src, pitch, nfields, out, out_stride, count, stream);
}

}  // namespace interpn
