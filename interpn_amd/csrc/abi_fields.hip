// Field sets (include/interpn_hip.h, "Field sets"): K value grids on one grid.  A set owns the field-major device
// copy of `vals`, K ordinary handles on slices of it (the per-field path: a loop of evaluations through them, with
// every tuned path the single handles have) and, for multilinear N = 2, 3, the fused kernel's table
// (linear_fields.h).  (C ABI internals, see abi_internal.h.)
#include <climits>

#include "abi_internal.h"

using namespace interpn;
using namespace interpn_abi;

struct interpn_hip_fields {
  int device = 0;
  int dtype = kF64;
  int ndims = 0;
  size_t nfields = 0;
  size_t field_stride = 0;        // elements from field to field in `vals`
  size_t field_elems = 0;         // elements of one field
  int per_line = 0;               // fused table: fields per line (P) and lines per cell
  size_t lines = 0;
  void* vals_owned = nullptr;     // device copy of the whole buffer when created from host memory
  const void* vals = nullptr;     // device, field-major
  std::vector<interpn_hip_interp*> sub;  // one handle per field
  void* table = nullptr;          // the fused kernel's table, or null: per-field only
  size_t table_bytes = 0;
  int fused = -1;                 // option: -1 automatic, 0 never, 1 wherever the table exists
  int last_path = INTERPN_HIP_FIELDS_PATH_PER_FIELD;
  bool sub_tables = true;         // the K handles have built their own re-laid tables (false: deferred)
  bool per_field_pending = false; // per-field evaluations since the last finish: every handle's status word counts
  std::mutex mu;                  // the deferred table build
  std::mutex host_mu;             // host evaluations share the staging below: serialised
  // host evaluation: one stream, the coordinates of a chunk and its K result rows on the device
  hipStream_t stream = nullptr;
  unsigned long long* kit_word = nullptr;
  void* host_obs = nullptr;
  void* host_out = nullptr;
  size_t host_points = 0;
};

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
  if (s->table && (s->fused == 1 || (s->fused < 0 && auto_takes_fused(s, npoints, hs, flags)))) {
    interpn_hip_interp* h0 = s->sub[0];  // its description carries the grid, the axes, the flavour and the options
    HIP_TRY(launch_linear_fields(h0->desc, s->table, (int)s->nfields, obs, out, out_stride, npoints, h0->first_bad, hs));
    mark_stream(h0, hs);
    s->last_path = INTERPN_HIP_FIELDS_PATH_FUSED;
    if (path_taken) *path_taken = INTERPN_HIP_FIELDS_PATH_FUSED;
    return INTERPN_HIP_OK;
  }
  if (!s->sub_tables && !(flags & INTERPN_HIP_EVAL_NO_ALLOC)) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(hs, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusActive; }
    if (cs == hipStreamCaptureStatusNone) {
      st = ensure_sub_tables(s);
      if (st) return st;
    }
  }
  const size_t elem = s->dtype == kF64 ? 8 : 4;
  s->per_field_pending = true;
  s->last_path = INTERPN_HIP_FIELDS_PATH_PER_FIELD;
  for (size_t f = 0; f < s->nfields; ++f) {
    st = interpn_hip_eval_device_ex(s->sub[f], obs, nobs, static_cast<char*>(out) + f * out_stride * elem, npoints, stream, flags,
                                    nullptr, nullptr);
    if (st) return st;
  }
  return INTERPN_HIP_OK;
}

int interpn_hip_fields_finish(interpn_hip_fields* s, void* stream, uint64_t* first_bad_index) {
  if (!s || s->sub.empty()) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  // fused evaluations report through the first handle's word; per-field ones through every handle's (the same index
  // in each: the cell search does not depend on the field)
  const size_t count = s->per_field_pending ? s->nfields : 1;
  s->per_field_pending = false;
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

void interpn_hip_fields_destroy(interpn_hip_fields* s) {
  if (!s) return;
  DeviceGuard guard(s->device);
  if (s->stream && hipStreamSynchronize(s->stream) != hipSuccess) (void)hipGetLastError();
  for (interpn_hip_interp* h : s->sub) interpn_hip_destroy(h);  // waits for the work enqueued through the set (stream marks)
  if (s->stream) pool_return_kit(s->device, s->stream, s->kit_word);
  pool_free(s->device, s->host_obs);
  pool_free(s->device, s->host_out);
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
