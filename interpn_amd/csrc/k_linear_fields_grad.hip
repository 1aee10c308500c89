// Field sets: the launcher of the fused value-and-Jacobian kernel (linear_fields_grad.h) on the set's fused table.
#include "linear_fields_grad.h"

namespace interpn {

template <typename T, int N, bool RECT, bool FMA>
static hipError_t launch_n(const GridDesc& g, const void* table, int nfields, const void* const* obs, void* out, size_t out_stride,
                           void* grad, size_t grad_stride, size_t npts, unsigned long long* first_bad, hipStream_t stream) {
  typedef FieldsLayout<T, N> L;
  FieldsGradArgs<T, N> a = {};
  a.table = static_cast<const unsigned char*>(table);
  a.out = static_cast<T*>(out);
  a.out_stride = out_stride;
  a.grad = static_cast<T*>(grad);
  a.grad_stride = grad_stride;
  a.first_bad = first_bad;
  a.npts = npts;
  a.nfields = nfields;
  a.groups = (unsigned)((nfields + L::P - 1) / L::P);
  unsigned acc = a.groups;
  for (int d = N - 1; d >= 0; --d) {
    a.obs[d] = static_cast<const T*>(obs[d]);
    a.start[d] = (T)g.start[d];
    a.step[d] = (T)g.step[d];
    a.n[d] = g.n[d];
    a.cstride[d] = acc;
    acc *= (unsigned)(g.n[d] - 1);
  }
  // LDS: the axis image of a rectilinear grid while it fits Thresholds::axis_lds (rect_args.h), then the waves' exchange
  // areas (P (N + 1) result rows each)
  size_t lds = 0;
  if constexpr (RECT) lds = (fill_axis_args<T, N>(g, a.ax, /*big_lds=*/false, /*records=*/true) + 15) & ~(size_t)15;
  lds += (size_t)(kBlock / 64) * FieldsGradLayout<T, N>::kWaveLds;
  if (lds > (size_t)64 << 10) return hipErrorInvalidValue;  // only with option axis_lds_kb beyond 34: 20 + 29.7 KiB at most otherwise
  g.tag.set("k_linear_fields_grad", {N, RECT, FMA}, 0b110u);
  hipLaunchKernelGGL((k_linear_fields_grad<T, N, RECT, FMA>), dim3(grid_blocks(npts, 1, g.cfg)), dim3(kBlock), lds, stream, a);
  return hipGetLastError();
}

hipError_t launch_linear_fields_grad(const GridDesc& g, const void* table, int nfields, const void* const* obs, void* out,
                                     size_t out_stride, void* grad, size_t grad_stride, size_t npts, unsigned long long* first_bad,
                                     hipStream_t stream) {
  if (npts == 0) return hipSuccess;
#define FIELDS_GRAD_CASE(T, N)                                                                                                       \
  if (g.kind == kRectilinear)                                                                                                        \
    return g.fma ? launch_n<T, N, true, true>(g, table, nfields, obs, out, out_stride, grad, grad_stride, npts, first_bad, stream)  \
                 : launch_n<T, N, true, false>(g, table, nfields, obs, out, out_stride, grad, grad_stride, npts, first_bad, stream); \
  return g.fma ? launch_n<T, N, false, true>(g, table, nfields, obs, out, out_stride, grad, grad_stride, npts, first_bad, stream)   \
               : launch_n<T, N, false, false>(g, table, nfields, obs, out, out_stride, grad, grad_stride, npts, first_bad, stream);
  if (g.ndims == 2) {
    if (g.dtype == kF64) { FIELDS_GRAD_CASE(double, 2) }
    FIELDS_GRAD_CASE(float, 2)
  }
  if (g.ndims == 3) {
    if (g.dtype == kF64) { FIELDS_GRAD_CASE(double, 3) }
    FIELDS_GRAD_CASE(float, 3)
  }
#undef FIELDS_GRAD_CASE
  return hipErrorInvalidValue;
}

}  // namespace interpn
