// Lattice evaluation: the observation points are the tensor product of N coordinate vectors (one per axis), results in
// C order with the last axis contiguous — re-gridding, `RegularGridInterpolator` on a meshgrid, refining a table.
//
// What a lattice shares between its points:
//   * everything the reference derives from ONE coordinate of ONE axis — cell index, normalized coordinate, the cubic
//     saturation class, the rectilinear spacing ratios — exists sum(m_d) times, not prod(m_d) * N times.  k_lattice_axes
//     computes it once per axis coordinate with the device functions the per-point kernels use (interpn_device.h) and
//     stores it as a record (below).
//   * the reference reduces dimension 0 first and dimension N-1 last (multilinear/regular.rs:366-403,
//     multicubic/regular.rs:368-421).  For one output row (all lattice indices but the last fixed) the partial results
//     after dims 0..N-2 depend only on the grid column k of the last axis: r[k], k < n_{N-1}.  k_lattice_rows computes
//     that line once per row into LDS; every output of the row is then ONE node of the last dimension over
//     r[loc .. loc + 1] (linear) or r[loc .. loc + 3] (cubic).  Operations and operands are those of interp_one, in its
//     order: the bits are the per-point kernels'.
//
// Traffic model of the row kernel (per output row, T = element type, F = 2 linear / 4 cubic, n = n_{N-1} grid points and
// m = m_{N-1} lattice coordinates along the last axis): F^(N-1) coalesced reads of n elements of the C-ordered `vals`
// (table rows that the rows in flight share: L2 hits), m record reads (16 to 64 bytes, the same m records for every row:
// L2 hits), m result stores — the only stream that reaches HBM: sizeof(T) per point against (N + 1) sizeof(T) for the
// per-point kernels on an expanded lattice.  Nodes: (F^(N-1) - 1) / (F - 1) per grid column plus one per point, instead
// of (F^N - 1) / (F - 1) per point.
//
// Launch shape: 256-thread persistent workgroups, ONE ROW PER WAVE (the row's records of dims 0..N-2 are wave-uniform
// and come through the scalar unit; a wave synchronises with itself only), four LDS lines per workgroup.
#pragma once

#include "interpn_device.h"
#include "interpn_host.h"

namespace interpn {

constexpr int kLatticeWaves = 4;                 // waves (= rows in flight, = LDS lines) per workgroup
constexpr int kLatticeBlock = 64 * kLatticeWaves;
constexpr size_t kLatticeMaxCoords = (size_t)1 << 31;  // sum of the axis lengths a call accepts (records and flags are indexed with 32 bits)

// Per-coordinate records.  `cls` = Sat | linear << 2 (linear: outside the grid under linearize_extrapolation).
template <typename T> struct LatticeRecLinear { T t; int loc; };
template <typename T> struct LatticeRecCubic { T tt; int loc; int cls; };
template <typename T> struct LatticeRecCubicRect { T t, r0, a0, c0, r1, a1, c1; int loc; int cls; };

template <typename T, int METHOD, bool RECT> struct LatticeRec { typedef LatticeRecLinear<T> type; };
template <typename T> struct LatticeRec<T, kCubic, false> { typedef LatticeRecCubic<T> type; };
template <typename T> struct LatticeRec<T, kCubic, true> { typedef LatticeRecCubicRect<T> type; };

inline size_t lattice_record_bytes(int method, int kind, size_t elem) {
  if (method == kLinear) return elem == 8 ? sizeof(LatticeRecLinear<double>) : sizeof(LatticeRecLinear<float>);
  if (kind == kRegular) return elem == 8 ? sizeof(LatticeRecCubic<double>) : sizeof(LatticeRecCubic<float>);
  return elem == 8 ? sizeof(LatticeRecCubicRect<double>) : sizeof(LatticeRecCubicRect<float>);
}

// One LDS line of the row kernel: n_{N-1} elements, rounded up to 16 bytes.
inline size_t lattice_line_bytes(size_t n_last, size_t elem) { return (n_last * elem + 15) & ~(size_t)15; }

enum LatticeMode : int { kLatticeAuto = -1, kLatticeNever = 0, kLatticeFused = 1 };

// Which path a lattice takes.  `covered`: the row kernel exists for (method, N); `fits`: its four lines fit `budget` bytes
// of LDS.  Automatic mode adds the two layout rules of DESIGN.md ("Lattice evaluation"):
//   rows   a wave owns a row, so a lattice needs rows to fill the device: prod(m_0 .. m_{N-2}) >= 4 waves x num_cus;
//   last   a row costs F^(N-1) reads per GRID column before its first output: n_{N-1} <= 4 max(m_{N-1}, 64).
struct LatticePlan {
  bool covered = false, fits = false, fused = false;
  size_t lds_bytes = 0;    // of a workgroup on the fused path (0 otherwise)
  size_t nrows = 0;        // prod(m_0 .. m_{N-2})
};
inline LatticePlan lattice_plan(int method, int ndims, size_t elem, const int* n, const size_t* m, size_t budget, int num_cus,
                                int mode) {
  LatticePlan p;
  p.covered = (method == kLinear || method == kCubic) && (ndims == 2 || ndims == 3);
  if (!p.covered) return p;
  const size_t n_last = (size_t)n[ndims - 1], m_last = m[ndims - 1];
  const size_t lds = (size_t)kLatticeWaves * lattice_line_bytes(n_last, elem);
  p.fits = lds <= budget;
  p.nrows = 1;
  for (int d = 0; d + 1 < ndims; ++d) p.nrows *= m[d];
  bool fused = p.fits && mode != kLatticeNever;
  for (int d = 0; d < ndims; ++d) fused = fused && m[d] < ((size_t)1 << 31);
  if (fused && mode == kLatticeAuto) {
    const size_t wide = m_last > 64 ? m_last : 64;
    fused = p.nrows >= (size_t)kLatticeWaves * (size_t)num_cus && n_last <= 4 * wide;
  }
  p.fused = fused;
  p.lds_bytes = fused ? lds : 0;
  return p;
}

// ---- Gradients on a lattice (lattice_grad.h, k_lattice_grad.hip) ---------------------------------------------------------
// A wave of k_lattice_grad_rows owns L lines where k_lattice_rows owns one: the value line and one line per gradient
// component (multilinear: N + 1, the last component's differences along the last axis being a line of their own;
// multicubic: N, the last component coming from the value line's derivative node).
inline int lattice_grad_lines(int method, int ndims) { return method == kLinear ? ndims + 1 : ndims; }
// The L lines of a wave lie packed, n_{N-1} elements each (a line needs its element's alignment only); the wave's part is
// rounded up to 16 bytes.  3-D f64 in 20 KiB: multilinear n_last <= 160 (4 waves x 4 lines x 1280 bytes), multicubic <= 213.
inline size_t lattice_grad_wave_bytes(int lines, size_t n_last, size_t elem) {
  return ((size_t)lines * n_last * elem + 15) & ~(size_t)15;
}

// Which path a value-and-gradient call takes on a lattice: lattice_plan's coverage, mode and automatic rules (carried
// over from the value kernel), `fits` for the L lines of a wave.
inline LatticePlan lattice_grad_plan(int method, int ndims, size_t elem, const int* n, const size_t* m, size_t budget, int num_cus,
                                     int mode) {
  LatticePlan p;
  p.covered = (method == kLinear || method == kCubic) && (ndims == 2 || ndims == 3);
  if (!p.covered) return p;
  const size_t n_last = (size_t)n[ndims - 1], m_last = m[ndims - 1];
  const size_t lds = (size_t)kLatticeWaves * lattice_grad_wave_bytes(lattice_grad_lines(method, ndims), n_last, elem);
  p.fits = lds <= budget;
  p.nrows = 1;
  for (int d = 0; d + 1 < ndims; ++d) p.nrows *= m[d];
  bool fused = p.fits && mode != kLatticeNever;
  for (int d = 0; d < ndims; ++d) fused = fused && m[d] < ((size_t)1 << 31);
  if (fused && mode == kLatticeAuto) {
    const size_t wide = m_last > 64 ? m_last : 64;
    fused = p.nrows >= (size_t)kLatticeWaves * (size_t)num_cus && n_last <= 4 * wide;
  }
  p.fused = fused;
  p.lds_bytes = fused ? lds : 0;
  return p;
}

// The LDS budget of the row kernel's lines: what the handle already grants rectilinear axis images
// (Thresholds::axis_lds, or option "axis_lds_kb").
inline size_t lattice_lds_budget(const LaunchConfig& c) {
  return c.axis_lds_kb >= 0 ? (size_t)c.axis_lds_kb * 1024 : thresholds(c).axis_lds;
}

// ---- Field sets on a lattice (k_lattice_fields.hip) ----------------------------------------------------------------------
// K fields of one grid on one lattice: the records of a lattice do not depend on the field, so one axes launch serves all
// of them, and k_lattice_fields_rows puts a field loop around k_lattice_rows' row.  Fields are processed in groups of G: a
// wave owns G lines (line f = dims 0..N-2 of field f0 + f reduced at every grid column); a lane then loads the last axis's
// record ONCE per output and evaluates one node per field of the group.  Two result layouts:
//   field-major   out[f * out_stride + p]: each field's row segment stored coalesced, as k_lattice_rows does.
//   fields-last   out[p * out_stride + f]: the wave stages a [64][G] tile in LDS (rows (G | 1) elements apart: an odd
//                 pitch keeps the lanes of a column off one bank) and stores its 64 G elements lane-contiguously.
// LDS of a workgroup and the group size:
//   wave_bytes(g) = g * lattice_line_bytes(n_{N-1}, elem) + (fields-last ? round16(64 * (g | 1) * elem) : 0)
//   G             = the largest g in 1 .. min(K, kLatticeFieldsCap) with kLatticeWaves * wave_bytes(g) <= budget, 0 if none
//   lds_bytes     = kLatticeWaves * wave_bytes(G)
// kLatticeFieldsCap = 8: what a larger group still saves is the last axis's record load, 1 / G of it per output and field,
// and at G = 8 a point's run of a fields-last row is already a whole 32-byte sector in f32 and a whole 64-byte request in
// f64, while the tile (4.5 KiB per wave in f64) has taken most of a wave's default 5 KiB share.  From the cost model, not
// from a measurement: no measured row has K > 4.
constexpr int kLatticeFieldsCap = 8;
enum LatticeFieldsLayout : int { kLatticeFieldMajor = 0, kLatticeFieldsLast = 1 };

inline size_t lattice_fields_tile_bytes(size_t g, size_t elem) { return ((size_t)64 * (g | 1) * elem + 15) & ~(size_t)15; }
inline size_t lattice_fields_wave_bytes(size_t n_last, size_t elem, size_t g, int layout) {
  return g * lattice_line_bytes(n_last, elem) + (layout == kLatticeFieldsLast ? lattice_fields_tile_bytes(g, elem) : 0);
}

// Which path a field set takes on a lattice.  Fused when lattice_plan says fused for the mode and a group of at least one
// field fits (field-major: exactly lattice_plan's `fits`; fields-last: the tile of one field on top).  Automatic mode adds
// nothing for a set.  A first form of the rule sent fields-last results with short runs per point (G != K and G * elem <
// 16: partial-sector stores) through the per-field path; measured, the fused kernel wins the rows that condition would
// have turned away (G = 1 of K = 3, 4) by 1.16 .. 1.38 against K single evaluations and a stack — what the per-field path
// amounts to there, plus a join — and by 1.69 .. 2.76 against the per-field path with expansion
// (profiles/fields_lattice_bench.json: ratio_baseline_over_fused, ratio_per_field_over_fused), so
// that condition is gone.
struct FieldsLatticePlan {
  bool fused = false;
  size_t group = 0;       // G on the fused path (0 otherwise)
  size_t lds_bytes = 0;   // of a workgroup on the fused path (0 otherwise)
};
inline FieldsLatticePlan fields_lattice_plan(int method, int ndims, size_t elem, const int* n, const size_t* m, size_t nfields,
                                             int layout, size_t budget, int num_cus, int mode) {
  FieldsLatticePlan p;
  const LatticePlan one = lattice_plan(method, ndims, elem, n, m, budget, num_cus, mode);
  if (!one.fused || nfields == 0) return p;
  const size_t n_last = (size_t)n[ndims - 1];
  const size_t top = nfields < (size_t)kLatticeFieldsCap ? nfields : (size_t)kLatticeFieldsCap;
  size_t g = 0;
  while (g < top && (size_t)kLatticeWaves * lattice_fields_wave_bytes(n_last, elem, g + 1, layout) <= budget) ++g;
  if (g == 0) return p;
  p.fused = true;
  p.group = g;
  p.lds_bytes = (size_t)kLatticeWaves * lattice_fields_wave_bytes(n_last, elem, g, layout);
  return p;
}

// ---- Field-set gradients on a lattice (lattice_fields_grad.h, k_lattice_fields_grad.hip) ---------------------------------
// The product of the two kernels above: k_lattice_fields_rows' field loop, groups and fields-last tile around
// k_lattice_grad_rows' L lines per field.  A wave owns G x L packed lines (field f of the group: lines f * L ..); per chunk
// of 64 outputs a lane loads the last axis's record, width and sign once and computes, per field of the group, the value
// and the N components.  Two result layouts (strides in elements):
//   field-major   out[f * out_stride + p], jac[(f * N + d) * jac_stride + p]: N + 1 coalesced stores per field.
//   fields-last   out[p * out_stride + f], jac[p * jac_stride + f * N + d]: the wave stages a [64] x P tile in LDS,
//                 P = (G * (N + 1)) | 1 (a point's G values first, then its G x N Jacobian elements; the odd pitch keeps
//                 the lanes of a column off one bank), and stores the values and then the Jacobian lane-contiguously.
// LDS of a workgroup and the group size:
//   wave_bytes(g) = round16(g * L * n_{N-1} * elem) + (fields-last ? round16(64 * ((g * (N + 1)) | 1) * elem) : 0)
//   G             = the largest g in 1 .. min(K, kLatticeFieldsCap) with kLatticeWaves * wave_bytes(g) <= budget, 0 if none
//   lds_bytes     = kLatticeWaves * wave_bytes(G)
// At the default 20 KiB (5120 bytes per wave) a fields-last f64 3-D call never has G > 2: the tile of three fields is
// 64 x 13 x 8 = 6656 bytes by itself, and the tile of two (4608) leaves room for lines of n_last <= 8 (multilinear) or 10
// (multicubic) only, so G = 1 is the rule there.  The tile of N + 1 results per field takes the room; "axis_lds_kb" is the knob.
inline size_t lattice_fields_grad_lines_bytes(int lines, size_t n_last, size_t elem, size_t g) {
  return (g * (size_t)lines * n_last * elem + 15) & ~(size_t)15;
}
inline size_t lattice_fields_grad_tile_pitch(size_t g, int ndims) { return (g * (size_t)(ndims + 1)) | 1; }
inline size_t lattice_fields_grad_wave_bytes(int lines, int ndims, size_t n_last, size_t elem, size_t g, int layout) {
  const size_t tile = ((size_t)64 * lattice_fields_grad_tile_pitch(g, ndims) * elem + 15) & ~(size_t)15;
  return lattice_fields_grad_lines_bytes(lines, n_last, elem, g) + (layout == kLatticeFieldsLast ? tile : 0);
}

// Which path a field set's value-and-Jacobian call takes on a lattice.  Fused when lattice_grad_plan says fused for the
// mode (coverage, the `lattice` option, the two automatic rules) and a group of at least one field fits.  No rule of its
// own: see DESIGN.md section 20 for what was and was not measured.
inline FieldsLatticePlan fields_lattice_grad_plan(int method, int ndims, size_t elem, const int* n, const size_t* m, size_t nfields,
                                                  int layout, size_t budget, int num_cus, int mode) {
  FieldsLatticePlan p;
  const LatticePlan one = lattice_grad_plan(method, ndims, elem, n, m, budget, num_cus, mode);
  if (!one.fused || nfields == 0) return p;
  const size_t n_last = (size_t)n[ndims - 1];
  const int lines = lattice_grad_lines(method, ndims);
  const size_t top = nfields < (size_t)kLatticeFieldsCap ? nfields : (size_t)kLatticeFieldsCap;
  size_t g = 0;
  while (g < top && (size_t)kLatticeWaves * lattice_fields_grad_wave_bytes(lines, ndims, n_last, elem, g + 1, layout) <= budget) ++g;
  if (g == 0) return p;
  p.fused = true;
  p.group = g;
  p.lds_bytes = (size_t)kLatticeWaves * lattice_fields_grad_wave_bytes(lines, ndims, n_last, elem, g, layout);
  return p;
}

// The lattice as the kernels see it (host arrays of at most kMaxDims entries).
struct LatticeShape {
  int ndims = 0;
  const void* axes[8] = {nullptr};   // device
  size_t m[8] = {0};
  unsigned rec_off[8] = {0};         // index of axis d's first record / flag: sum of m[0 .. d)
  unsigned long long weight[8] = {0};  // prod of m[e], e > d: the flat index step of axis d
  size_t coords = 0;                 // sum of m
  size_t npoints = 0;
};

// k_lattice.hip
// Records of every axis coordinate into `recs` (lattice_record_bytes each; fused path), and on regular grids the
// bad-coordinate flags (`bad`, one byte per coordinate, may be null) with the atomicMin of the flat index of the first
// failing lattice point into `first_bad`.  `recs` null: flags and first_bad only (expanded path; every method).
hipError_t launch_lattice_axes(const GridDesc& g, const LatticeShape& s, void* recs, unsigned char* bad,
                               unsigned long long* first_bad, hipStream_t stream);
hipError_t launch_lattice_rows(const GridDesc& g, const LatticeShape& s, const void* recs, void* out, size_t lds_bytes,
                               hipStream_t stream);
// SoA coordinates of the lattice points [begin, begin + count) into dst[d][0 .. count); a coordinate flagged in `bad`
// (may be null) is replaced by the grid's first coordinate, so that the evaluation of the slice never reports a
// slice-relative failing index (the axes kernel has reported the lattice's).
hipError_t launch_lattice_expand(const GridDesc& g, const LatticeShape& s, const unsigned char* bad, void* const* dst,
                                 size_t begin, size_t count, hipStream_t stream);
// k_lattice_fields.hip
// The rows of `nfields` fields (field f at g.vals + f * field_stride elements) from the records of launch_lattice_axes:
// groups of `group` fields, `lds_bytes` as fields_lattice_plan gives them; `layout`, `out_stride` as above.
hipError_t launch_lattice_fields_rows(const GridDesc& g, const LatticeShape& s, const void* recs, size_t field_stride, size_t nfields,
                                      size_t group, void* out, size_t out_stride, int layout, size_t lds_bytes, hipStream_t stream);

// k_lattice_grad.hip
// The rows' values and gradient components (grad[d]: device, npoints elements each) from the records of
// launch_lattice_axes; `lds_bytes` as lattice_grad_plan gives them.
hipError_t launch_lattice_grad_rows(const GridDesc& g, const LatticeShape& s, const void* recs, void* out, void* const* grad,
                                    size_t lds_bytes, hipStream_t stream);

// k_lattice_fields_grad.hip
// The rows' values and Jacobian of `nfields` fields (field f at g.vals + f * field_stride elements) from the records of
// launch_lattice_axes: groups of `group` fields, `lds_bytes` as fields_lattice_grad_plan gives them; `layout` and the two
// strides as above.
hipError_t launch_lattice_fields_grad_rows(const GridDesc& g, const LatticeShape& s, const void* recs, size_t field_stride,
                                           size_t nfields, size_t group, void* out, size_t out_stride, void* jac, size_t jac_stride,
                                           int layout, size_t lds_bytes, hipStream_t stream);

}  // namespace interpn
