// Field-set gradients on a lattice (lattice_fields_grad.h): the launcher of k_lattice_fields_grad_rows, 64 instantiations
// ({f64, f32} x {multilinear, multicubic} x N = 2, 3 x {regular, rectilinear} x {fma, no fma} x {field-major, fields-last}).
#include "lattice_fields_grad.h"

namespace interpn {

template <typename T, int METHOD, int N, bool RECT, bool FMA, bool LAST>
static hipError_t launch_k(const GridDesc& g, const LatticeShape& s, const void* recs, size_t field_stride, size_t nfields,
                           size_t group, void* out, size_t out_stride, void* jac, size_t jac_stride, size_t lds_bytes,
                           hipStream_t stream) {
  LatticeFieldsGradRowsArgs<T, N> fa;
  LatticeRowsArgs<T, N>& a = fa.r;
  a.vals = static_cast<const T*>(g.vals);
  a.recs = recs;
  a.out = static_cast<T*>(out);
  a.nrows = 1;
  unsigned acc = 1;
  for (int d = N - 1; d >= 0; --d) {
    a.m[d] = (unsigned)s.m[d];
    a.rec_off[d] = s.rec_off[d];
    a.stride[d] = acc;
    acc *= (unsigned)g.n[d];
    if (d < N - 1) a.nrows *= s.m[d];
    fa.grid[d] = RECT ? static_cast<const T*>(g.grid[d]) : nullptr;
    fa.step[d] = (T)g.step[d];
  }
  a.n_last = g.n[N - 1];
  a.line_bytes = 0;
  fa.jac = static_cast<T*>(jac);
  fa.field_stride = field_stride;
  fa.out_stride = out_stride;
  fa.jac_stride = jac_stride;
  fa.nfields = (unsigned)nfields;
  fa.group = (unsigned)group;
  const int lines = lattice_grad_lines(METHOD, N);
  const int layout = LAST ? kLatticeFieldsLast : kLatticeFieldMajor;
  fa.tile_off = (unsigned)lattice_fields_grad_lines_bytes(lines, (size_t)g.n[N - 1], sizeof(T), group);
  fa.wave_bytes = (unsigned)lattice_fields_grad_wave_bytes(lines, N, (size_t)g.n[N - 1], sizeof(T), group, layout);
  if ((size_t)kLatticeWaves * fa.wave_bytes > lds_bytes) return hipErrorInvalidValue;  // the plan's bytes hold the waves' areas
  const unsigned long long want = (a.nrows + kLatticeWaves - 1) / kLatticeWaves;
  const unsigned long long cap = (unsigned long long)g.cfg.num_cus * (unsigned long long)g.cfg.blocks_per_cu;
  const unsigned blocks = (unsigned)(want < cap ? want : cap);
  g.tag.set("k_lattice_fields_grad_rows", {METHOD, N, RECT, FMA, LAST}, 0b11100u);
  hipLaunchKernelGGL((k_lattice_fields_grad_rows<T, METHOD, N, RECT, FMA, LAST>), dim3(blocks), dim3(kLatticeBlock), lds_bytes, stream,
                     fa);
  return hipGetLastError();
}

template <typename T, int METHOD, int N, bool RECT, bool FMA>
static hipError_t launch_l(const GridDesc& g, const LatticeShape& s, const void* recs, size_t field_stride, size_t nfields,
                           size_t group, void* out, size_t out_stride, void* jac, size_t jac_stride, int layout, size_t lds_bytes,
                           hipStream_t stream) {
  return layout == kLatticeFieldsLast
             ? launch_k<T, METHOD, N, RECT, FMA, true>(g, s, recs, field_stride, nfields, group, out, out_stride, jac, jac_stride,
                                                       lds_bytes, stream)
             : launch_k<T, METHOD, N, RECT, FMA, false>(g, s, recs, field_stride, nfields, group, out, out_stride, jac, jac_stride,
                                                        lds_bytes, stream);
}

template <typename T, int METHOD, int N>
static hipError_t launch_n(const GridDesc& g, const LatticeShape& s, const void* recs, size_t field_stride, size_t nfields,
                           size_t group, void* out, size_t out_stride, void* jac, size_t jac_stride, int layout, size_t lds_bytes,
                           hipStream_t stream) {
#define LATTICE_FIELDS_GRAD_FLAVOUR(RECT, FMA) \
  launch_l<T, METHOD, N, RECT, FMA>(g, s, recs, field_stride, nfields, group, out, out_stride, jac, jac_stride, layout, lds_bytes, stream)
  if (g.kind == kRegular) return g.fma ? LATTICE_FIELDS_GRAD_FLAVOUR(false, true) : LATTICE_FIELDS_GRAD_FLAVOUR(false, false);
  return g.fma ? LATTICE_FIELDS_GRAD_FLAVOUR(true, true) : LATTICE_FIELDS_GRAD_FLAVOUR(true, false);
#undef LATTICE_FIELDS_GRAD_FLAVOUR
}

template <typename T>
static hipError_t launch_t(const GridDesc& g, const LatticeShape& s, const void* recs, size_t field_stride, size_t nfields,
                           size_t group, void* out, size_t out_stride, void* jac, size_t jac_stride, int layout, size_t lds_bytes,
                           hipStream_t stream) {
#define LATTICE_FIELDS_GRAD_CASE(METHOD, N) \
  if (g.method == METHOD && g.ndims == N) \
    return launch_n<T, METHOD, N>(g, s, recs, field_stride, nfields, group, out, out_stride, jac, jac_stride, layout, lds_bytes, stream);
  LATTICE_FIELDS_GRAD_CASE(kLinear, 2)
  LATTICE_FIELDS_GRAD_CASE(kLinear, 3)
  LATTICE_FIELDS_GRAD_CASE(kCubic, 2)
  LATTICE_FIELDS_GRAD_CASE(kCubic, 3)
#undef LATTICE_FIELDS_GRAD_CASE
  return hipErrorInvalidValue;
}

hipError_t launch_lattice_fields_grad_rows(const GridDesc& g, const LatticeShape& s, const void* recs, size_t field_stride,
                                           size_t nfields, size_t group, void* out, size_t out_stride, void* jac, size_t jac_stride,
                                           int layout, size_t lds_bytes, hipStream_t stream) {
  if (group < 1 || group > nfields || group > (size_t)kLatticeFieldsCap || nfields > 0xFFFFFFFFull) return hipErrorInvalidValue;
  if (layout != kLatticeFieldMajor && layout != kLatticeFieldsLast) return hipErrorInvalidValue;
  if (layout == kLatticeFieldMajor ? (out_stride < s.npoints || jac_stride < s.npoints)
                                   : (out_stride < nfields || jac_stride < nfields * (size_t)s.ndims))
    return hipErrorInvalidValue;
  for (int d = 0; d < s.ndims; ++d)
    if (s.m[d] >= ((size_t)1 << 31)) return hipErrorInvalidValue;
  if (s.npoints == 0) return hipSuccess;
  return g.dtype == kF64
             ? launch_t<double>(g, s, recs, field_stride, nfields, group, out, out_stride, jac, jac_stride, layout, lds_bytes, stream)
             : launch_t<float>(g, s, recs, field_stride, nfields, group, out, out_stride, jac, jac_stride, layout, lds_bytes, stream);
}

}  // namespace interpn
