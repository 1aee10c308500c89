// Field sets: the table builder and the launcher of the fused multilinear kernel (linear_fields.h).
#include "linear_fields.h"

namespace interpn {

bool fields_geometry(size_t elem_size, int ndims, const size_t* dims, size_t nfields, FieldsGeometry* out) {
  if ((elem_size != 4 && elem_size != 8) || (ndims != 2 && ndims != 3) || !dims || nfields == 0 || !out) return false;
  const size_t per_line = (size_t)128 / (((size_t)1 << ndims) * elem_size);
  FieldsGeometry geo;
  geo.fields_per_line = (int)per_line;
  geo.lines_per_point = (nfields + per_line - 1) / per_line;
  geo.cells = 1;
  for (int d = 0; d < ndims; ++d) {
    if (dims[d] < 2) return false;
    if (__builtin_mul_overflow(geo.cells, dims[d] - 1, &geo.cells)) return false;
  }
  size_t lines;
  if (__builtin_mul_overflow(geo.cells, geo.lines_per_point, &lines) || __builtin_mul_overflow(lines, (size_t)128, &geo.table_bytes))
    return false;
  *out = geo;
  return true;
}

template <typename T, int N>
static hipError_t build_n(const GridDesc& g, const void* vals, size_t field_stride, int nfields, void* table, hipStream_t stream) {
  typedef FieldsLayout<T, N> L;
  FieldsBuildDims<N> dims;
  size_t acc = 1, cells = 1;
  for (int d = N - 1; d >= 0; --d) {
    dims.ncell[d] = (unsigned)(g.n[d] - 1);
    dims.stride[d] = acc;
    acc *= (size_t)g.n[d];
    cells *= (size_t)(g.n[d] - 1);
  }
  const unsigned groups = (unsigned)((nfields + L::P - 1) / L::P);
  const size_t total = cells * groups * L::EPL;
  hipLaunchKernelGGL((k_fields_build<T, N>), dim3(one_pass_blocks(total, 4)), dim3(kBlock), 0, stream, static_cast<const T*>(vals),
                     field_stride, nfields, groups, dims, static_cast<T*>(table), total);
  return hipGetLastError();
}

hipError_t build_fields_table(const GridDesc& g, const void* vals, size_t field_stride, int nfields, void* table, hipStream_t stream) {
  if (g.ndims == 2)
    return g.dtype == kF64 ? build_n<double, 2>(g, vals, field_stride, nfields, table, stream)
                           : build_n<float, 2>(g, vals, field_stride, nfields, table, stream);
  if (g.ndims == 3)
    return g.dtype == kF64 ? build_n<double, 3>(g, vals, field_stride, nfields, table, stream)
                           : build_n<float, 3>(g, vals, field_stride, nfields, table, stream);
  return hipErrorInvalidValue;
}

template <typename T, int N, bool RECT, bool FMA>
static hipError_t launch_n(const GridDesc& g, const void* table, int nfields, const void* const* obs, void* out, size_t out_stride,
                           size_t npts, unsigned long long* first_bad, hipStream_t stream) {
  typedef FieldsLayout<T, N> L;
  FieldsArgs<T, N> a = {};
  a.table = static_cast<const unsigned char*>(table);
  a.out = static_cast<T*>(out);
  a.out_stride = out_stride;
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
  // LDS: the axis image of a rectilinear grid while it fits Thresholds::axis_lds (rect_args.h), then the waves' exchange areas
  size_t lds = 0;
  if constexpr (RECT) lds = (fill_axis_args<T, N>(g, a.ax, /*big_lds=*/false, /*records=*/true) + 15) & ~(size_t)15;
  lds += (size_t)(kBlock / 64) * L::kWaveLds;
  g.tag.set("k_linear_fields", {N, RECT, FMA}, 0b110u);
  hipLaunchKernelGGL((k_linear_fields<T, N, RECT, FMA>), dim3(grid_blocks(npts, 1, g.cfg)), dim3(kBlock), lds, stream, a);
  return hipGetLastError();
}

hipError_t launch_linear_fields(const GridDesc& g, const void* table, int nfields, const void* const* obs, void* out,
                                size_t out_stride, size_t npts, unsigned long long* first_bad, hipStream_t stream) {
  if (npts == 0) return hipSuccess;
#define FIELDS_CASE(T, N)                                                                                                   \
  if (g.kind == kRectilinear)                                                                                               \
    return g.fma ? launch_n<T, N, true, true>(g, table, nfields, obs, out, out_stride, npts, first_bad, stream)            \
                 : launch_n<T, N, true, false>(g, table, nfields, obs, out, out_stride, npts, first_bad, stream);          \
  return g.fma ? launch_n<T, N, false, true>(g, table, nfields, obs, out, out_stride, npts, first_bad, stream)             \
               : launch_n<T, N, false, false>(g, table, nfields, obs, out, out_stride, npts, first_bad, stream);
  if (g.ndims == 2) {
    if (g.dtype == kF64) { FIELDS_CASE(double, 2) }
    FIELDS_CASE(float, 2)
  }
  if (g.ndims == 3) {
    if (g.dtype == kF64) { FIELDS_CASE(double, 3) }
    FIELDS_CASE(float, 3)
  }
#undef FIELDS_CASE
  return hipErrorInvalidValue;
}

}  // namespace interpn
