// Field sets (include/interpn_hip.h, "Field sets"): K value grids on one grid.  A set owns the field-major device
// copy of `vals`, K ordinary handles on slices of it (the per-field path: a loop of evaluations through them, with
// every tuned path the single handles have) and, for multilinear N = 2, 3, the fused kernel's table
// (linear_fields.h).  Behind the column form, the point-major form of the same sets ("Point-major field sets": the fused
// kernel of linear_fields_points.h on that table, or slices that are de-interleaved, evaluated by the column form and
// joined).  The lattice form of a set lives in abi_fields_lattice.hip.  (C ABI internals, see abi_internal.h.)
#include <climits>

#include "abi_internal.h"

using namespace interpn;
using namespace interpn_abi;

namespace {

struct DeferTables {
  explicit DeferTables(bool on) { t_defer_tables = on; }
  ~DeferTables() { t_defer_tables = false; }
};

long long env_number(const char* name, long long fallback) {
  const char* env = getenv(name);
  if (!env || !*env) return fallback;
  char* end = nullptr;
  const long long v = strtoll(env, &end, 0);
  return (end == env || *end != 0) ? fallback : v;
}

}  // namespace

namespace interpn_abi {
// The K handles' own tables, once (the per-field path's first use outside capture).
int ensure_sub_tables(interpn_hip_fields* s) {
  std::lock_guard<std::mutex> lk(s->mu);
  if (s->sub_tables) return INTERPN_HIP_OK;
  for (interpn_hip_interp* h : s->sub) {
    const int st = maybe_build_bricks(h);
    if (st) return st;
  }
  s->sub_tables = true;
  return INTERPN_HIP_OK;
}
}  // namespace interpn_abi

namespace {

// Which path an evaluation of `npoints` points on `stream` takes when the caller leaves it to the set (fused = -1).
// Measured (profiles/fields_bench.json): the fused kernel runs at the Infinity Cache's rate for
// unordered lines, about 2.1 ms per 1e8 lines whatever they hold, so it wins by what a line carries.
//   1. Lines less than 3/4 full (K = 2 where P >= 4): K single-field lines cost less than one half-empty fused line
//      (per-field / fused = 0.60 .. 0.86) -> per field.
//   2. Two fields per line (f64, N = 3), a field's grid within Thresholds::table_l2_sized, and a batch for which the
//      per-field path takes the sweep kernel (sweep_applies on a field's handle: from Thresholds-sized batches on, outside
//      capture): that kernel feeds its lines from the L2 in table order, 0.9 ms per field and 1e8 points against 1.07
//      (0.82 .. 0.87, rectilinear 0.85 .. 1.01) -> per field.  This needs the handles' own tables, so they are built here
//      for batches of Thresholds::binned_points_min points or more unless the call may not allocate.
//   3. Everything else — small batches, f32 and 2-D f64 with full lines, grids beyond the L2 — fused (1.13 .. 1.62).
bool auto_takes_fused(interpn_hip_fields* s, size_t npoints, hipStream_t stream, unsigned flags) {
  if (4 * s->nfields < 3 * s->lines * (size_t)s->per_line) return false;
  const GridDesc& g0 = s->sub[0]->desc;
  const Thresholds th = thresholds(g0.cfg);
  const size_t elem = s->dtype == kF64 ? 8 : 4;
  if (s->per_line == 2 && s->field_elems * elem <= th.table_l2_sized && npoints >= th.binned_points_min && g0.cfg.sweep != 0) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cs) != hipSuccess) { (void)hipGetLastError(); return true; }
    if (cs != hipStreamCaptureStatusNone) return true;  // captured per-field evaluations run in place, not the sweep kernel
    if (!s->sub_tables && ((flags & INTERPN_HIP_EVAL_NO_ALLOC) || ensure_sub_tables(s) != INTERPN_HIP_OK)) return true;
    if (sweep_applies(g0, npoints) >= 2) return false;
  }
  return true;
}

// Everything the two creators share.  `prod`: elements of one field (0: not computable — `validate` then reports
// why); `make_sub(vals_f, handle)` creates the handle of one field from its device slice.
template <typename T, typename Validate, typename MakeSub>
int create_fields(int method, const size_t* dims, size_t ndims, const T* vals, size_t nvals, size_t nfields,
                  size_t field_stride, int vals_mem, int device, interpn_hip_fields** out, Validate validate, MakeSub make_sub) {
  if (!out) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  const int flavour = method & (INTERPN_HIP_FLAVOUR_FMA | INTERPN_HIP_FLAVOUR_NO_FMA);
  if (flavour == (INTERPN_HIP_FLAVOUR_FMA | INTERPN_HIP_FLAVOUR_NO_FMA)) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  const int m = method & ~(INTERPN_HIP_FLAVOUR_FMA | INTERPN_HIP_FLAVOUR_NO_FMA);
  if (m != kLinear && m != kCubic && m != kNearest) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  if (vals_mem != INTERPN_HIP_MEM_HOST && vals_mem != INTERPN_HIP_MEM_DEVICE) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  if (nfields == 0) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  size_t prod = 0;
  if (dims && ndims <= 8 && checked_product(dims, ndims, &prod)) {
    size_t need;
    if (field_stride < prod) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
    if (__builtin_mul_overflow(nfields - 1, field_stride, &need) || __builtin_add_overflow(need, prod, &need) || nvals < need)
      return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  }
  int st = validate(m, prod);
  if (st) return st;
  if (!vals) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  int dev;
  st = resolve_device(device, &dev);
  if (st) return st;
  DeviceGuard guard(dev);
  if (!guard.ok()) return INTERPN_HIP_ERR_NO_DEVICE;
  interpn_hip_fields* s = new (std::nothrow) interpn_hip_fields();
  if (!s) return INTERPN_HIP_ERR_OUT_OF_MEMORY;
  s->device = dev;
  s->dtype = sizeof(T) == 8 ? kF64 : kF32;
  s->ndims = (int)ndims;
  s->nfields = nfields;
  s->field_stride = field_stride;
  s->field_elems = prod;
  auto fail = [&](int status) {
    interpn_hip_fields_destroy(s);
    return status;
  };
  if (vals_mem == INTERPN_HIP_MEM_DEVICE) {
    s->vals = vals;
  } else {
    hipError_t e = pool_alloc(dev, &s->vals_owned, nvals * sizeof(T));
    if (e == hipSuccess) e = hipMemcpy(s->vals_owned, vals, nvals * sizeof(T), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(hip_fail(e));
    s->vals = s->vals_owned;
  }
  // The fused table: multilinear N = 2, 3, line indices in 32 bits, and a quarter of the free memory at most.
  const long long env_fused = env_number("INTERPN_HIP_FIELDS_FUSED", -1);
  if (env_fused >= -1 && env_fused <= 1) s->fused = (int)env_fused;
  FieldsGeometry geo;
  if (m == kLinear && s->fused != 0 && nfields <= (size_t)INT_MAX && fields_geometry(sizeof(T), (int)ndims, dims, nfields, &geo) &&
      geo.cells * geo.lines_per_point < 0xFFFFFFFFull) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = (size_t)8 << 30; }
    size_t budget = free_b / 4;
    const long long env_budget = env_number("INTERPN_HIP_FIELDS_TABLE_BUDGET", -1);
    if (env_budget >= 0 && (size_t)env_budget < budget) budget = (size_t)env_budget;
    if (geo.table_bytes <= budget) {
      if (pool_alloc(dev, &s->table, geo.table_bytes) == hipSuccess) {
        GridDesc g;
        g.dtype = s->dtype;
        g.ndims = (int)ndims;
        for (size_t d = 0; d < ndims; ++d) g.n[d] = (int)dims[d];
        hipError_t e = build_fields_table(g, s->vals, field_stride, (int)nfields, s->table, nullptr);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess) return fail(hip_fail(e));
        s->table_bytes = geo.table_bytes;
        s->per_line = geo.fields_per_line;
        s->lines = geo.lines_per_point;
      } else {
        (void)hipGetLastError();
        s->table = nullptr;
      }
    }
  }
  s->sub_tables = s->table == nullptr;
  s->sub.reserve(nfields);
  for (size_t f = 0; f < nfields; ++f) {
    DeferTables defer(!s->sub_tables);
    interpn_hip_interp* h = nullptr;
    st = make_sub(static_cast<const T*>(s->vals) + f * field_stride, prod, dev, &h);
    if (st) return fail(st);
    s->sub.push_back(h);
  }
  *out = s;
  return INTERPN_HIP_OK;
}

// Whether the column form evaluates `npoints` points on `stream` with the fused kernel (option "fused" and its rule).
bool columns_take_fused(interpn_hip_fields* s, size_t npoints, hipStream_t stream, unsigned flags) {
  return s->table && (s->fused == 1 || (s->fused < 0 && auto_takes_fused(s, npoints, stream, flags)));
}

// The column form's evaluation on validated arguments (the current device is the set's): one fused launch, or K
// evaluations through the K handles.
int eval_columns(interpn_hip_fields* s, bool fused, const void* const* obs, void* out, size_t out_stride, size_t npoints,
                 hipStream_t hs, unsigned flags) {
  if (fused) {
    interpn_hip_interp* h0 = s->sub[0];  // its description carries the grid, the axes, the flavour and the options
    HIP_TRY(launch_linear_fields(h0->desc, s->table, (int)s->nfields, obs, out, out_stride, npoints, h0->first_bad, hs));
    mark_stream(h0, hs);
    s->last_path = INTERPN_HIP_FIELDS_PATH_FUSED;
    return INTERPN_HIP_OK;
  }
  if (!s->sub_tables && !(flags & INTERPN_HIP_EVAL_NO_ALLOC)) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(hs, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusActive; }
    if (cs == hipStreamCaptureStatusNone) {
      const int st = ensure_sub_tables(s);
      if (st) return st;
    }
  }
  const size_t elem = s->dtype == kF64 ? 8 : 4;
  s->per_field_pending = true;
  s->last_path = INTERPN_HIP_FIELDS_PATH_PER_FIELD;
  for (size_t f = 0; f < s->nfields; ++f) {
    const int st = interpn_hip_eval_device_ex(s->sub[f], obs, (size_t)s->ndims, static_cast<char*>(out) + f * out_stride * elem, npoints,
                                              hs, flags, nullptr, nullptr);
    if (st) return st;
  }
  return INTERPN_HIP_OK;
}

// ---- point-major form ---------------------------------------------------------------------------------------------------

using Slot = interpn_hip_interp::BinSlot;

// Points per slice of the split path: the slice's N coordinate arrays and K result rows together stay within what
// kExpandSliceBytes allows the coordinate arrays of a handle's slice; whole multiples of 256 points (slices then begin
// 16-byte aligned in every array: sweep evaluation), 256 at least.
size_t points_slice(const interpn_hip_fields* s, size_t npoints) {
  const size_t elem = s->dtype == kF64 ? 8 : 4;
  size_t slice = kExpandSliceBytes / (((size_t)s->ndims + s->nfields) * elem);
  const long long opt = s->sub[0]->desc.cfg.points_slice;  // testing
  if (opt > 0) slice = (size_t)opt;
  slice &= ~(size_t)255;
  if (slice < 256) slice = 256;
  return npoints < slice ? npoints : slice;
}

// Bytes in front of the arrays: a parked first-failing index per handle.
size_t points_head(const interpn_hip_fields* s) { return align_up(s->nfields * sizeof(unsigned long long), 256); }

size_t points_need(const interpn_hip_fields* s, size_t npoints) {
  const size_t elem = s->dtype == kF64 ? 8 : 4;
  return points_head(s) + ((size_t)s->ndims + s->nfields) * align_up(points_slice(s, npoints) * elem, 256);
}

// The automatic rule of the point-major form for a set that has the table.  The alternative to the
// fused kernel is the split path, whose column evaluation is the better of k_linear_fields and the per-field path
// (auto_takes_fused) plus the split and the join: 2 (N + K) more elements read and written per point.  auto_takes_fused
// prefers the per-field path in two classes, by 0.60 .. 0.86 (lines less than 3/4 full) and 0.82 .. 1.01 (two fields per
// line against the sweep kernel, which a slice is too small for anyway) of k_linear_fields' time; the two extra passes
// cost more than either margin.  Measured (profiles/fields_points_bench.json, 48 rows: 3-D 64^3 and 128^3 f64 / f32,
// rectilinear 64^3 f64, 2-D 1000^2 f64; K = 2, 3, 4, 8; 4e6 and 1e8 points): fused / split = 0.41 .. 0.63 in every row,
// the rows of both classes included (K = 2 with P >= 4: 0.41 .. 0.59; 64^3 f64 at 1e8: 0.47 .. 0.61).  So the rule has no
// per-field class and no batch threshold left: fused wherever the table exists.  Not measured: other K, 2-D f32,
// rectilinear f32 and 2-D, batches below 4e6 points, padded rows.
bool points_auto_takes_fused(const interpn_hip_fields* s) { return s->table != nullptr; }

// INTERPN_HIP_FIELDS_POINTS_PATH_* for this call, or -1: option points_path = 1 on a set without the table.
int choose_points_path(const interpn_hip_fields* s) {
  if (s->points_path == 1) return s->table ? INTERPN_HIP_FIELDS_POINTS_PATH_FUSED : -1;
  if (s->points_path == 2) return INTERPN_HIP_FIELDS_POINTS_PATH_SPLIT;
  if (!s->table || s->fused == 0) return INTERPN_HIP_FIELDS_POINTS_PATH_SPLIT;  // fused = 0: the set's fused kernels are off
  return points_auto_takes_fused(s) ? INTERPN_HIP_FIELDS_POINTS_PATH_FUSED : INTERPN_HIP_FIELDS_POINTS_PATH_SPLIT;
}

// What both entry points check, in this order (that of the handles' points_checks), before any device work.
int points_checks(const interpn_hip_fields* s, const void* pts, size_t stride, size_t npoints, const void* out, size_t out_stride,
                  bool* nothing, int* path) {
  *nothing = false;
  if (!s || s->sub.empty()) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  if (stride < (size_t)s->ndims) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  if (out_stride < s->nfields) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  if (npoints == 0) { *nothing = true; return INTERPN_HIP_OK; }
  if (!pts || !out) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  if (npoints > (~(size_t)0) / 8 / stride || npoints > (~(size_t)0) / 8 / out_stride)
    return INTERPN_HIP_ERR_INVALID_ARGUMENT;  // both blocks' bytes fit size_t
  *path = choose_points_path(s);
  return *path < 0 ? INTERPN_HIP_ERR_UNSUPPORTED : INTERPN_HIP_OK;
}

// The split path: a scratch block from the first field's handle (reserved blocks only under capture, allocation unless
// NO_ALLOC otherwise) holds the parked words, the slice's N coordinate arrays and its K result rows.  Per slice:
// k_split_points, the column form (fused or per field by its own option and rule), k_join_fields.  The slice's kernels
// count failing points from the slice's start, so around every slice but the first the word of EVERY handle that
// interpn_hip_fields_finish will read — one on the fused path, all K on the per-field path — is parked and `begin` added
// afterwards: the minimum finish takes is then an index of the whole call.
int points_split(interpn_hip_fields* s, const void* pts, size_t stride, size_t npoints, void* out, size_t out_stride,
                 hipStream_t stream, unsigned flags) {
  interpn_hip_interp* h0 = s->sub[0];
  const GridDesc& g = h0->desc;
  const size_t elem = s->dtype == kF64 ? 8 : 4;
  const size_t nd = (size_t)s->ndims;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusActive; }
  const bool capturing = cs != hipStreamCaptureStatusNone;
  const size_t need = points_need(s, npoints);
  int why = INTERPN_HIP_WHY_NONE;
  Slot* slot = capturing ? take_slot_captured(h0, need, stream) : take_bin_slot(h0, need, stream, !(flags & INTERPN_HIP_EVAL_NO_ALLOC), &why);
  if (!slot) return INTERPN_HIP_ERR_OUT_OF_MEMORY;  // no block reserved (interpn_hip_fields_reserve_points) and none may be made
  claim_slot(h0, slot);
  unsigned char* scratch = static_cast<unsigned char*>(slot->scratch);
  unsigned long long* saved = reinterpret_cast<unsigned long long*>(scratch);
  const size_t slice = points_slice(s, npoints);
  const size_t pitch = align_up(slice * elem, 256);
  void* col[8] = {nullptr};
  for (size_t d = 0; d < nd; ++d) col[d] = scratch + points_head(s) + d * pitch;
  unsigned char* rows = scratch + points_head(s) + nd * pitch;
  hipError_t err = hipSuccess;
  int st = INTERPN_HIP_OK;
  for (size_t begin = 0; begin < npoints && err == hipSuccess && st == INTERPN_HIP_OK; begin += slice) {
    const size_t count = npoints - begin < slice ? npoints - begin : slice;
    err = launch_split_points(g, static_cast<const char*>(pts) + begin * stride * elem, stride, col, count, stream);
    if (err != hipSuccess) break;
    const bool fused = columns_take_fused(s, count, stream, flags);
    const size_t words = (begin && !fused) ? s->nfields : (begin ? 1 : 0);
    for (size_t f = 0; f < words && err == hipSuccess; ++f) err = launch_points_bad_begin(s->sub[f]->first_bad, saved + f, stream);
    if (err != hipSuccess) break;  // (a word parked without its counterpart: the sequence failed as a whole)
    st = eval_columns(s, fused, col, rows, pitch / elem, count, stream, flags);
    for (size_t f = 0; f < words; ++f) {  // also behind a failed slice: the parked words go back
      const hipError_t e2 = launch_points_bad_end(s->sub[f]->first_bad, saved + f, (unsigned long long)begin, stream);
      if (err == hipSuccess) err = e2;
    }
    if (err == hipSuccess && st == INTERPN_HIP_OK)
      err = launch_join_fields(g, rows, pitch / elem, s->nfields, static_cast<char*>(out) + begin * out_stride * elem, out_stride, count,
                               stream);
  }
  if (capturing) release_slot_captured(h0, slot);
  else release_bin_slot(h0, slot, stream, false);
  if (err != hipSuccess || st != INTERPN_HIP_OK) {
    (void)hipGetLastError();
    std::lock_guard<std::mutex> lk(h0->marks_mu);
    h0->sync_device_at_destroy = true;  // part of the sequence may be in flight without a mark behind it
    return err != hipSuccess ? hip_fail(err) : st;
  }
  mark_stream(h0, stream);
  return INTERPN_HIP_OK;
}

// One block of points on device memory.  Arguments are validated; the current device is the set's.
int points_device(interpn_hip_fields* s, int path, const void* pts, size_t stride, size_t npoints, void* out, size_t out_stride,
                  hipStream_t stream, unsigned flags) {
  if (path == INTERPN_HIP_FIELDS_POINTS_PATH_FUSED) {
    interpn_hip_interp* h0 = s->sub[0];
    HIP_TRY(launch_linear_fields_points(h0->desc, s->table, (int)s->nfields, pts, stride, out, out_stride, npoints, h0->first_bad, stream));
    mark_stream(h0, stream);
    s->last_path = INTERPN_HIP_FIELDS_PATH_FUSED;
  } else {
    const int st = points_split(s, pts, stride, npoints, out, out_stride, stream, flags);
    if (st) return st;
  }
  s->last_points_path = path;
  return INTERPN_HIP_OK;
}

}  // namespace

extern "C" {

#define DEFINE_FIELDS(T, SUFFIX)                                                                                       \
  int interpn_hip_create_fields_regular_##SUFFIX(int method, const size_t* dims, size_t ndims, const T* starts,       \
                                                 size_t nstarts, const T* steps, size_t nsteps, const T* vals,        \
                                                 size_t nvals, size_t nfields, size_t field_stride, int vals_mem,     \
                                                 int linearize_extrapolation, int device, interpn_hip_fields** fields) { \
    return create_fields<T>(                                                                                          \
        method, dims, ndims, vals, nvals, nfields, field_stride, vals_mem, device, fields,                            \
        [&](int m, size_t prod) { return validate_regular<T>(m, dims, ndims, starts, nstarts, steps, nsteps, prod); }, \
        [&](const T* v, size_t prod, int dev, interpn_hip_interp** h) {                                               \
          return create_regular<T>(method, dims, ndims, starts, nstarts, steps, nsteps, v, prod,                      \
                                   INTERPN_HIP_MEM_DEVICE, linearize_extrapolation, dev, h);                          \
        });                                                                                                           \
  }                                                                                                                    \
  int interpn_hip_create_fields_rectilinear_##SUFFIX(int method, const T* const* grids, const size_t* grid_lens,      \
                                                     size_t ngrids, const T* vals, size_t nvals, size_t nfields,      \
                                                     size_t field_stride, int vals_mem, int linearize_extrapolation,  \
                                                     int device, interpn_hip_fields** fields) {                       \
    return create_fields<T>(                                                                                          \
        method, grid_lens, ngrids, vals, nvals, nfields, field_stride, vals_mem, device, fields,                      \
        [&](int m, size_t prod) { return validate_rectilinear<T>(m, grids, grid_lens, ngrids, prod); },               \
        [&](const T* v, size_t prod, int dev, interpn_hip_interp** h) {                                               \
          return create_rectilinear<T>(method, grids, grid_lens, ngrids, v, prod, INTERPN_HIP_MEM_DEVICE,             \
                                       linearize_extrapolation, dev, h);                                              \
        });                                                                                                           \
  }
DEFINE_FIELDS(double, f64)
DEFINE_FIELDS(float, f32)

int interpn_hip_fields_eval_device(interpn_hip_fields* s, const void* const* obs, size_t nobs, void* out, size_t out_stride,
                                   size_t npoints, void* stream, unsigned flags, int* path_taken) {
  if (path_taken) *path_taken = INTERPN_HIP_FIELDS_PATH_PER_FIELD;
  if (!s || s->sub.empty() || (!obs && nobs)) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  if (flags & ~(unsigned)INTERPN_HIP_EVAL_NO_ALLOC) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  int st = validate_obs(s->sub[0]->desc, nullptr, nobs, npoints);
  if (st) return st;
  if (npoints == 0) return INTERPN_HIP_OK;
  if (!out || out_stride < npoints) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  for (size_t i = 0; i < nobs; ++i)
    if (!obs[i]) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  DeviceGuard guard(s->device);
  if (!guard.ok()) return INTERPN_HIP_ERR_NO_DEVICE;
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const bool fused = columns_take_fused(s, npoints, hs, flags);
  st = eval_columns(s, fused, obs, out, out_stride, npoints, hs, flags);
  if (st == INTERPN_HIP_OK && fused && path_taken) *path_taken = INTERPN_HIP_FIELDS_PATH_FUSED;
  return st;
}

int interpn_hip_fields_finish(interpn_hip_fields* s, void* stream, uint64_t* first_bad_index) {
  if (!s || s->sub.empty()) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  // fused evaluations report through the first handle's word; per-field ones through every handle's (the same index
  // in each: the cell search does not depend on the field)
  const size_t count = s->per_field_pending ? s->nfields : 1;
  s->per_field_pending = false;
  if (count > 1 && count <= (size_t)kMaxStatusWords) {
    // the K words behind ONE command and one wait: the status kernel delivers their minimum (abi_host.hip)
    unsigned long long* words[kMaxStatusWords];
    for (size_t f = 0; f < count; ++f) words[f] = s->sub[f]->first_bad;
    const int st = finish_words(s->sub[0], static_cast<hipStream_t>(stream), words, (int)count, first_bad_index);
    if (st >= 0) return st;
  }
  int error = INTERPN_HIP_OK;
  uint64_t best = ~(uint64_t)0;
  for (size_t f = 0; f < count; ++f) {
    uint64_t bad = 0;
    const int st = interpn_hip_finish(s->sub[f], stream, &bad);
    if (st == s->sub[f]->desc.unrep_status) best = bad < best ? bad : best;
    else if (st != INTERPN_HIP_OK && error == INTERPN_HIP_OK) error = st;
  }
  if (error) return error;
  if (best != ~(uint64_t)0) {
    if (first_bad_index) *first_bad_index = best;
    return s->sub[0]->desc.unrep_status;
  }
  return INTERPN_HIP_OK;
}

int interpn_hip_fields_eval_host(interpn_hip_fields* s, const void* const* obs, const size_t* obs_lens, size_t nobs, void* out,
                                 size_t out_stride, size_t nout) {
  if (!s || s->sub.empty() || (!obs && nobs) || (!obs_lens && nobs)) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  int st = validate_obs(s->sub[0]->desc, obs_lens, nobs, nout);
  if (st) return st;
  if (nout == 0) return INTERPN_HIP_OK;
  if (!out || out_stride < nout) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  for (size_t i = 0; i < nobs; ++i)
    if (!obs[i]) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  DeviceGuard guard(s->device);
  if (!guard.ok()) return INTERPN_HIP_ERR_NO_DEVICE;
  const size_t elem = s->dtype == kF64 ? 8 : 4;
  const long long opt_chunk = s->sub[0]->desc.cfg.host_chunk;
  size_t chunk = opt_chunk >= 1 ? (size_t)opt_chunk : ((size_t)2 << 20);
  if (chunk > nout) chunk = nout;
  std::lock_guard<std::mutex> host_lock(s->host_mu);
  if (!s->stream) HIP_TRY(pool_take_kit(s->device, &s->stream, &s->kit_word));
  if (s->host_points < chunk) {
    HIP_TRY(hipStreamSynchronize(s->stream));
    pool_free(s->device, s->host_obs);
    pool_free(s->device, s->host_out);
    s->host_obs = s->host_out = nullptr;
    s->host_points = 0;
    HIP_TRY(pool_alloc(s->device, &s->host_obs, (size_t)s->ndims * chunk * elem));
    HIP_TRY(pool_alloc(s->device, &s->host_out, s->nfields * chunk * elem));
    s->host_points = chunk;
  }
  const size_t cap = s->host_points;
  char* dev_obs_base = static_cast<char*>(s->host_obs);
  char* dev_out = static_cast<char*>(s->host_out);
  const void* dev_obs[8];
  for (size_t begin = 0; begin < nout; begin += chunk) {
    const size_t count = nout - begin < chunk ? nout - begin : chunk;
    // the chunk's coordinates cross PCIe once, whatever the number of fields
    for (int d = 0; d < s->ndims; ++d) {
      char* dst = dev_obs_base + (size_t)d * cap * elem;
      HIP_TRY(hipMemcpyAsync(dst, static_cast<const char*>(obs[d]) + begin * elem, count * elem, hipMemcpyHostToDevice, s->stream));
      dev_obs[d] = dst;
    }
    st = interpn_hip_fields_eval_device(s, dev_obs, nobs, dev_out, cap, count, s->stream, 0u, nullptr);
    if (st) return st;
    uint64_t bad = 0;
    st = interpn_hip_fields_finish(s, s->stream, &bad);
    const bool failed = st == s->sub[0]->desc.unrep_status;
    if (st && !failed) return st;
    // the reference stops at the first failing point: rows written in front of it, untouched behind it
    const size_t good = failed ? (size_t)bad : count;
    if (good)
      for (size_t f = 0; f < s->nfields; ++f)
        HIP_TRY(hipMemcpyAsync(static_cast<char*>(out) + (f * out_stride + begin) * elem, dev_out + f * cap * elem, good * elem,
                               hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (failed) return st;
  }
  return INTERPN_HIP_OK;
}

int interpn_hip_fields_eval_points_device(interpn_hip_fields* s, const void* pts, size_t point_stride, size_t npoints, void* out,
                                          size_t out_stride, void* stream, unsigned flags, int* path_taken) {
  if (path_taken) *path_taken = INTERPN_HIP_FIELDS_POINTS_PATH_SPLIT;
  if (flags & ~(unsigned)INTERPN_HIP_EVAL_NO_ALLOC) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  bool nothing = false;
  int path = INTERPN_HIP_FIELDS_POINTS_PATH_SPLIT;
  const int st0 = points_checks(s, pts, point_stride, npoints, out, out_stride, &nothing, &path);
  if (st0 || nothing) return st0;
  DeviceGuard guard(s->device);
  if (!guard.ok()) return INTERPN_HIP_ERR_NO_DEVICE;
  const int st = points_device(s, path, pts, point_stride, npoints, out, out_stride, static_cast<hipStream_t>(stream), flags);
  if (st == INTERPN_HIP_OK && path_taken) *path_taken = path;
  return st;
}

int interpn_hip_fields_reserve_points(interpn_hip_fields* s, size_t npoints, int nstreams) {
  if (!s || s->sub.empty() || nstreams < 0) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  if ((size_t)nstreams > interpn_hip_interp::kMaxBinSlots) nstreams = (int)interpn_hip_interp::kMaxBinSlots;
  if (npoints == 0 || nstreams == 0) return INTERPN_HIP_OK;
  DeviceGuard guard(s->device);
  if (!guard.ok()) return INTERPN_HIP_ERR_NO_DEVICE;
  return reserve_slots(s->sub[0], points_need(s, npoints), nstreams);
}

int interpn_hip_fields_eval_points_host(interpn_hip_fields* s, const void* pts, size_t point_stride, size_t npoints, void* out,
                                        size_t out_stride) {
  bool nothing = false;
  int path = INTERPN_HIP_FIELDS_POINTS_PATH_SPLIT;
  const int st0 = points_checks(s, pts, point_stride, npoints, out, out_stride, &nothing, &path);
  if (st0 || nothing) return st0;
  DeviceGuard guard(s->device);
  if (!guard.ok()) return INTERPN_HIP_ERR_NO_DEVICE;
  const size_t elem = s->dtype == kF64 ? 8 : 4;
  const size_t nd = (size_t)s->ndims, k = s->nfields;
  const long long opt_chunk = s->sub[0]->desc.cfg.host_chunk;
  size_t chunk = opt_chunk >= 1 ? (size_t)opt_chunk : ((size_t)2 << 20);
  if (chunk > npoints) chunk = npoints;
  // wide records or many fields would make a chunk large: its rows and its results within 256 MiB each
  const size_t widest = point_stride > k ? point_stride : k;
  const size_t cap = ((size_t)256 << 20) / (widest * elem);
  if (chunk > cap) chunk = cap ? cap : 1;
  std::lock_guard<std::mutex> host_lock(s->host_mu);
  if (!s->stream) HIP_TRY(pool_take_kit(s->device, &s->stream, &s->kit_word));
  const size_t rows_bytes = align_up(chunk * point_stride * elem, 256);
  void* block = nullptr;  // the chunk's rows, then its packed result rows
  if (pool_alloc(s->device, &block, rows_bytes + chunk * k * elem) != hipSuccess) { (void)hipGetLastError(); return INTERPN_HIP_ERR_OUT_OF_MEMORY; }
  char* results = static_cast<char*>(block) + rows_bytes;
  hipError_t err = hipSuccess;
  int st = INTERPN_HIP_OK;
  for (size_t begin = 0; begin < npoints && err == hipSuccess && st == INTERPN_HIP_OK; begin += chunk) {
    const size_t count = npoints - begin < chunk ? npoints - begin : chunk;
    // one copy of the interleaved rows; the last row ends with its last coordinate
    err = hipMemcpyAsync(block, static_cast<const char*>(pts) + begin * point_stride * elem, ((count - 1) * point_stride + nd) * elem,
                         hipMemcpyHostToDevice, s->stream);
    if (err != hipSuccess) break;
    st = points_device(s, path, block, point_stride, count, results, k, s->stream, 0u);
    if (st) break;
    uint64_t bad = 0;
    st = interpn_hip_fields_finish(s, s->stream, &bad);
    const bool failed = st == s->sub[0]->desc.unrep_status;
    if (st && !failed) break;
    // the reference stops at the first failing point: the rows in front of it are written, everything else is left as it
    // was — the caller's elements behind a row's first K too
    const size_t good = failed ? (size_t)bad : count;
    char* dst = static_cast<char*>(out) + begin * out_stride * elem;
    if (good && out_stride == k) err = hipMemcpyAsync(dst, results, good * k * elem, hipMemcpyDeviceToHost, s->stream);
    else if (good) err = hipMemcpy2DAsync(dst, out_stride * elem, results, k * elem, k * elem, good, hipMemcpyDeviceToHost, s->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(s->stream);
  }
  (void)hipStreamSynchronize(s->stream);  // nothing in flight touches the block when it goes back to the pool
  pool_free(s->device, block);
  if (err != hipSuccess) return hip_fail(err);
  return st;
}

void interpn_hip_fields_destroy(interpn_hip_fields* s) {
  if (!s) return;
  DeviceGuard guard(s->device);
  if (s->stream && hipStreamSynchronize(s->stream) != hipSuccess) (void)hipGetLastError();
  for (interpn_hip_interp* h : s->sub) interpn_hip_destroy(h);  // waits for the work enqueued through the set (stream marks)
  if (s->stream) pool_return_kit(s->device, s->stream, s->kit_word);
  pool_free(s->device, s->host_obs);
  pool_free(s->device, s->host_out);
  pool_free(s->device, s->host_grad);
  pool_free(s->device, s->table);
  pool_free(s->device, s->vals_owned);
  delete s;
}

size_t interpn_hip_fields_count(const interpn_hip_fields* s) { return s ? s->nfields : 0; }
int interpn_hip_fields_ndims(const interpn_hip_fields* s) { return s ? s->ndims : 0; }
int interpn_hip_fields_elem_size(const interpn_hip_fields* s) { return s ? (s->dtype == kF64 ? 8 : 4) : 0; }
int interpn_hip_fields_device(const interpn_hip_fields* s) { return s ? s->device : -1; }

int interpn_hip_fields_kernel_name(const interpn_hip_fields* s, char* buf, size_t buflen) {
  if (!s || s->sub.empty()) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  return interpn_hip_kernel_name(s->sub[0], buf, buflen);  // the fused launch tags the first handle's description
}

int interpn_hip_fields_set_option(interpn_hip_fields* s, const char* name, long long value) {
  if (!s || !name) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  if (!strcmp(name, "fused")) {
    if (value < -1 || value > 1) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
    s->fused = (int)value;
    return INTERPN_HIP_OK;
  }
  if (!strcmp(name, "points_path")) {
    if (value != -1 && value != 1 && value != 2) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
    s->points_path = (int)value;
    return INTERPN_HIP_OK;
  }
  for (interpn_hip_interp* h : s->sub) {
    const int st = interpn_hip_set_option(h, name, value);
    if (st) return st;
  }
  return INTERPN_HIP_OK;
}

int interpn_hip_fields_get_option(const interpn_hip_fields* s, const char* name, long long* value) {
  if (!s || !name || !value || s->sub.empty()) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  if (!strcmp(name, "fused")) { *value = s->fused; return INTERPN_HIP_OK; }
  if (!strcmp(name, "fused_table_bytes")) { *value = s->table ? (long long)s->table_bytes : 0; return INTERPN_HIP_OK; }
  if (!strcmp(name, "nfields")) { *value = (long long)s->nfields; return INTERPN_HIP_OK; }
  if (!strcmp(name, "last_path")) { *value = s->last_path; return INTERPN_HIP_OK; }
  if (!strcmp(name, "points_path")) { *value = s->points_path; return INTERPN_HIP_OK; }
  if (!strcmp(name, "last_points_path")) { *value = s->last_points_path; return INTERPN_HIP_OK; }
  // (the set's own, not the first handle's: a per-field lattice evaluation leaves "fused" or "expanded" there)
  if (!strcmp(name, "last_lattice_path")) { *value = s->last_lattice_path; return INTERPN_HIP_OK; }
  if (!strcmp(name, "last_lattice_group")) { *value = s->last_lattice_group; return INTERPN_HIP_OK; }
  if (!strncmp(name, "evals_", 6)) {  // the per-field path evaluates through every handle: their counters, summed
    long long sum = 0;
    for (const interpn_hip_interp* h : s->sub) {
      long long v = 0;
      const int st = interpn_hip_get_option(h, name, &v);
      if (st) return st;
      sum += v;
    }
    *value = sum;
    return INTERPN_HIP_OK;
  }
  return interpn_hip_get_option(s->sub[0], name, value);
}

int interpn_hip_fields_layout(size_t elem_size, size_t ndims, const size_t* dims, size_t nfields, int* fields_per_line,
                              size_t* lines_per_point, size_t* table_bytes) {
  FieldsGeometry geo;
  if (ndims > 8 || !fields_geometry(elem_size, (int)ndims, dims, nfields, &geo)) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  if (fields_per_line) *fields_per_line = geo.fields_per_line;
  if (lines_per_point) *lines_per_point = geo.lines_per_point;
  if (table_bytes) *table_bytes = geo.table_bytes;
  return INTERPN_HIP_OK;
}

}  // extern "C"
