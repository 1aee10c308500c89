// Point-major gradients of a field set: the launcher of the fused kernel (linear_fields_points_grad.h) on the set's table.
#include "linear_fields_points_grad.h"

namespace interpn {

template <typename T, int N, bool RECT, bool FMA>
static hipError_t launch_n(const GridDesc& g, const void* table, int nfields, const void* pts, size_t stride, void* out,
                           size_t out_stride, void* jac, size_t jac_stride, size_t npts, unsigned long long* first_bad,
                           hipStream_t stream) {
  typedef FieldsLayout<T, N> L;
  typedef FieldsPointsGradLayout<T, N, RECT> PL;
  FieldsPointsGradArgs<T, N> a = {};
  a.table = static_cast<const unsigned char*>(table);
  a.pts = static_cast<const T*>(pts);
  a.stride = stride;
  a.out = static_cast<T*>(out);
  a.out_stride = out_stride;
  a.jac = static_cast<T*>(jac);
  a.jac_stride = jac_stride;
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
  if (lds > (size_t)64 << 10) return hipErrorInvalidValue;  // only with option axis_lds_kb beyond 27: 20 + 37 KiB at most otherwise
  g.tag.set("k_linear_fields_points_grad", {N, RECT, FMA}, 0b110u);
  hipLaunchKernelGGL((k_linear_fields_points_grad<T, N, RECT, FMA>), dim3(grid_blocks(npts, 1, g.cfg)), dim3(kBlock), lds, stream, a);
  return hipGetLastError();
}

hipError_t launch_linear_fields_points_grad(const GridDesc& g, const void* table, int nfields, const void* pts, size_t stride,
                                            void* out, size_t out_stride, void* jac, size_t jac_stride, size_t npts,
                                            unsigned long long* first_bad, hipStream_t stream) {
  if (stride < (size_t)g.ndims || nfields < 1 || out_stride < (size_t)nfields || jac_stride < (size_t)nfields * (size_t)g.ndims)
    return hipErrorInvalidValue;
  if (npts == 0) return hipSuccess;
#define FIELDS_POINTS_GRAD_CASE(T, N)                                                                                          \
  if (g.kind == kRectilinear)                                                                                                  \
    return g.fma ? launch_n<T, N, true, true>(g, table, nfields, pts, stride, out, out_stride, jac, jac_stride, npts, first_bad, stream)    \
                 : launch_n<T, N, true, false>(g, table, nfields, pts, stride, out, out_stride, jac, jac_stride, npts, first_bad, stream);  \
  return g.fma ? launch_n<T, N, false, true>(g, table, nfields, pts, stride, out, out_stride, jac, jac_stride, npts, first_bad, stream)     \
               : launch_n<T, N, false, false>(g, table, nfields, pts, stride, out, out_stride, jac, jac_stride, npts, first_bad, stream);
  if (g.ndims == 2) {
    if (g.dtype == kF64) { FIELDS_POINTS_GRAD_CASE(double, 2) }
    FIELDS_POINTS_GRAD_CASE(float, 2)
  }
  if (g.ndims == 3) {
    if (g.dtype == kF64) { FIELDS_POINTS_GRAD_CASE(double, 3) }
    FIELDS_POINTS_GRAD_CASE(float, 3)
  }
#undef FIELDS_POINTS_GRAD_CASE
  return hipErrorInvalidValue;
}

}  // namespace interpn
