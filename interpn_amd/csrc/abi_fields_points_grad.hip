// Point-major gradients of a field set (include/interpn_hip.h, "Point-major gradients of a field set"): the points as one
// (n, N) array, the K values as one (n, K) array and the Jacobian as one (n, K, N) array.  One launch of
// k_linear_fields_points_grad on the set's fused table (linear_fields_points_grad.h), or slices that are de-interleaved,
// evaluated by the column form (interpn_hip_fields_eval_grad_device) and joined.  (C ABI internals, see abi_internal.h.)
#include "abi_internal.h"

using namespace interpn;
using namespace interpn_abi;

namespace {

using Slot = interpn_hip_interp::BinSlot;

// Points per slice of the split path: the slice's N coordinate arrays, K value rows and K * N component rows together stay
// within what kExpandSliceBytes allows the coordinate arrays of a handle's slice; whole multiples of 256 points, 256 at least
// (the rule of the value form's points_slice, abi_fields.hip, for N + K (N + 1) arrays).
size_t slice_points(const interpn_hip_fields* s, size_t npoints) {
  const size_t elem = s->dtype == kF64 ? 8 : 4;
  const size_t nd = (size_t)s->ndims;
  size_t slice = kExpandSliceBytes / ((nd + s->nfields * (nd + 1)) * elem);
  const long long opt = s->sub[0]->desc.cfg.points_slice;  // testing
  if (opt > 0) slice = (size_t)opt;
  slice &= ~(size_t)255;
  if (slice < 256) slice = 256;
  return npoints < slice ? npoints : slice;
}

// Bytes in front of the arrays: a parked first-failing index per handle.
size_t scratch_head(const interpn_hip_fields* s) { return align_up(s->nfields * sizeof(unsigned long long), 256); }

size_t scratch_need(const interpn_hip_fields* s, size_t npoints) {
  const size_t elem = s->dtype == kF64 ? 8 : 4;
  const size_t nd = (size_t)s->ndims;
  return scratch_head(s) + (nd + s->nfields * (nd + 1)) * align_up(slice_points(s, npoints) * elem, 256);
}

// The automatic rule for a set that has the table.  The split path moves 2 (N + K + K N) more
// elements per point through the split and the two joins around the column kernel, which streams the same N + K + K N.
// Measured (profiles/fields_points_grad_bench.json, 13 rows at 1e7 points; fused / split): 0.44 .. 0.62 in every row but
// the two of 3-D 64^3 f64 K = 8: 0.98 regular and 0.96 rectilinear in the record, 1.10 and 1.06 in an earlier run of the
// same kernel — P = 2 there, so a point's 24-element Jacobian row is written in four runs of 6 elements by four line
// groups, and its 8 values in four runs of 2.  That class, two fields per line and four line groups or more (3-D f64,
// K >= 7), is level at best and goes to the split path; K = 5, 6 (three groups) are not measured and stay with K = 3 (two
// groups: 0.53, 0.54).
bool auto_takes_fused(const interpn_hip_fields* s) { return s->table != nullptr && !(s->per_line == 2 && s->lines >= 4); }

// INTERPN_HIP_FIELDS_POINTS_PATH_* for this call, or -1: option points_path = 1 on a set without the table.
int choose_path(const interpn_hip_fields* s) {
  if (s->points_path == 1) return s->table ? INTERPN_HIP_FIELDS_POINTS_PATH_FUSED : -1;
  if (s->points_path == 2) return INTERPN_HIP_FIELDS_POINTS_PATH_SPLIT;
  if (!s->table || s->fused == 0) return INTERPN_HIP_FIELDS_POINTS_PATH_SPLIT;  // fused = 0: the set's fused kernels are off
  return auto_takes_fused(s) ? INTERPN_HIP_FIELDS_POINTS_PATH_FUSED : INTERPN_HIP_FIELDS_POINTS_PATH_SPLIT;
}

// What both entry points check before any device work, in the order the header gives (`flags`: the device form's; the
// host form passes 0).
int checks(const interpn_hip_fields* s, const void* pts, size_t stride, size_t npoints, const void* out, size_t out_stride,
           const void* jac, size_t jac_stride, unsigned flags, bool* nothing, int* path) {
  *nothing = false;
  if (!s || s->sub.empty()) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  const int method = s->sub[0]->desc.method;
  if (method != kLinear && method != kCubic) return INTERPN_HIP_ERR_UNSUPPORTED;  // nearest: no gradient form
  const size_t nd = (size_t)s->ndims;
  if (stride < nd || out_stride < s->nfields || jac_stride < s->nfields * nd) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  if (npoints == 0) { *nothing = true; return INTERPN_HIP_OK; }
  if (!pts || !out || !jac) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  const size_t most = (~(size_t)0) / 8;
  if (npoints > most / stride || npoints > most / out_stride || npoints > most / jac_stride)
    return INTERPN_HIP_ERR_INVALID_ARGUMENT;  // the three blocks' bytes fit size_t
  if (flags & ~(unsigned)INTERPN_HIP_EVAL_NO_ALLOC) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  *path = choose_path(s);
  return *path < 0 ? INTERPN_HIP_ERR_UNSUPPORTED : INTERPN_HIP_OK;
}

// The split path: a scratch block from the first field's handle (reserved blocks only under capture, allocation unless
// NO_ALLOC otherwise) holds the parked words, the slice's N coordinate arrays, its K value rows and its K * N component
// rows.  Per slice: k_split_points, the column form (fused or per field by its own option and rule), k_join_fields for the
// K value rows and once more, with K * N "fields", for the component rows — row f * N + d of the column form is element
// f * N + d of the point's Jacobian row.  The slice's kernels count failing points from the slice's start, so around every
// slice but the first the word of EVERY handle that interpn_hip_fields_finish will read — one on the column form's fused
// path, all K on its per-field path — is parked and `begin` added afterwards, as the value form's points_split does.
int split(interpn_hip_fields* s, const void* pts, size_t stride, size_t npoints, void* out, size_t out_stride, void* jac,
          size_t jac_stride, hipStream_t stream, unsigned flags) {
  interpn_hip_interp* h0 = s->sub[0];
  const GridDesc& g = h0->desc;
  const size_t elem = s->dtype == kF64 ? 8 : 4;
  const size_t nd = (size_t)s->ndims, k = s->nfields;
  const bool capturing = stream_capturing(stream);
  const size_t need = scratch_need(s, npoints);
  int why = INTERPN_HIP_WHY_NONE;
  Slot* slot = capturing ? take_slot_captured(h0, need, stream) : take_bin_slot(h0, need, stream, !(flags & INTERPN_HIP_EVAL_NO_ALLOC), &why);
  if (!slot) return INTERPN_HIP_ERR_OUT_OF_MEMORY;  // no block reserved (interpn_hip_fields_reserve_points_grad) and none may be made
  claim_slot(h0, slot);
  unsigned char* scratch = static_cast<unsigned char*>(slot->scratch);
  unsigned long long* saved = reinterpret_cast<unsigned long long*>(scratch);
  const size_t slice = slice_points(s, npoints);
  const size_t pitch = align_up(slice * elem, 256);
  void* col[8] = {nullptr};
  for (size_t d = 0; d < nd; ++d) col[d] = scratch + scratch_head(s) + d * pitch;
  unsigned char* vrows = scratch + scratch_head(s) + nd * pitch;
  unsigned char* grows = vrows + k * pitch;
  hipError_t err = hipSuccess;
  int st = INTERPN_HIP_OK;
  for (size_t begin = 0; begin < npoints && err == hipSuccess && st == INTERPN_HIP_OK; begin += slice) {
    const size_t count = npoints - begin < slice ? npoints - begin : slice;
    err = launch_split_points(g, static_cast<const char*>(pts) + begin * stride * elem, stride, col, count, stream);
    if (err != hipSuccess) break;
    const size_t words = begin ? (grad_takes_fused(s) ? 1 : k) : 0;
    for (size_t f = 0; f < words && err == hipSuccess; ++f) err = launch_points_bad_begin(s->sub[f]->first_bad, saved + f, stream);
    if (err != hipSuccess) break;  // (a word parked without its counterpart: the sequence failed as a whole)
    st = interpn_hip_fields_eval_grad_device(s, col, nd, vrows, pitch / elem, grows, pitch / elem, count, stream, flags, nullptr);
    for (size_t f = 0; f < words; ++f) {  // also behind a failed slice: the parked words go back
      const hipError_t e2 = launch_points_bad_end(s->sub[f]->first_bad, saved + f, (unsigned long long)begin, stream);
      if (err == hipSuccess) err = e2;
    }
    if (err == hipSuccess && st == INTERPN_HIP_OK)
      err = launch_join_fields(g, vrows, pitch / elem, k, static_cast<char*>(out) + begin * out_stride * elem, out_stride, count, stream);
    if (err == hipSuccess && st == INTERPN_HIP_OK)
      err = launch_join_fields(g, grows, pitch / elem, k * nd, static_cast<char*>(jac) + begin * jac_stride * elem, jac_stride, count,
                               stream);
  }
  if (capturing) release_slot_captured(h0, slot);
  else release_bin_slot(h0, slot, stream, false);
  if (err != hipSuccess || st != INTERPN_HIP_OK) return fail_sequence(h0, err, st);
  mark_stream(h0, stream);
  return INTERPN_HIP_OK;
}

// One block of points on device memory.  Arguments are validated; the current device is the set's.
int points_grad_device(interpn_hip_fields* s, int path, const void* pts, size_t stride, size_t npoints, void* out, size_t out_stride,
                       void* jac, size_t jac_stride, hipStream_t stream, unsigned flags) {
  if (path == INTERPN_HIP_FIELDS_POINTS_PATH_FUSED) {
    interpn_hip_interp* h0 = s->sub[0];
    HIP_TRY(launch_linear_fields_points_grad(h0->desc, s->table, (int)s->nfields, pts, stride, out, out_stride, jac, jac_stride,
                                             npoints, h0->first_bad, stream));
    mark_stream(h0, stream);
    s->last_path = INTERPN_HIP_FIELDS_PATH_FUSED;
  } else {
    const int st = split(s, pts, stride, npoints, out, out_stride, jac, jac_stride, stream, flags);
    if (st) return st;
  }
  s->last_points_path = path;
  return INTERPN_HIP_OK;
}

}  // namespace

extern "C" {

int interpn_hip_fields_eval_points_grad_device(interpn_hip_fields* s, const void* pts, size_t point_stride, size_t npoints, void* out,
                                               size_t out_stride, void* jac, size_t jac_stride, void* stream, unsigned flags,
                                               int* path_taken) {
  if (path_taken) *path_taken = INTERPN_HIP_FIELDS_POINTS_PATH_SPLIT;
  bool nothing = false;
  int path = INTERPN_HIP_FIELDS_POINTS_PATH_SPLIT;
  const int st0 = checks(s, pts, point_stride, npoints, out, out_stride, jac, jac_stride, flags, &nothing, &path);
  if (st0 || nothing) return st0;
  DeviceGuard guard(s->device);
  if (!guard.ok()) return INTERPN_HIP_ERR_NO_DEVICE;
  const int st = points_grad_device(s, path, pts, point_stride, npoints, out, out_stride, jac, jac_stride,
                                    static_cast<hipStream_t>(stream), flags);
  if (st == INTERPN_HIP_OK && path_taken) *path_taken = path;
  return st;
}

int interpn_hip_fields_reserve_points_grad(interpn_hip_fields* s, size_t npoints, int nstreams) {
  if (!s || s->sub.empty() || nstreams < 0) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  if ((size_t)nstreams > interpn_hip_interp::kMaxBinSlots) nstreams = (int)interpn_hip_interp::kMaxBinSlots;
  if (npoints == 0 || nstreams == 0) return INTERPN_HIP_OK;
  DeviceGuard guard(s->device);
  if (!guard.ok()) return INTERPN_HIP_ERR_NO_DEVICE;
  return reserve_slots(s->sub[0], scratch_need(s, npoints), nstreams);
}

int interpn_hip_fields_eval_points_grad_host(interpn_hip_fields* s, const void* pts, size_t point_stride, size_t npoints, void* out,
                                             size_t out_stride, void* jac, size_t jac_stride) {
  bool nothing = false;
  int path = INTERPN_HIP_FIELDS_POINTS_PATH_SPLIT;
  const int st0 = checks(s, pts, point_stride, npoints, out, out_stride, jac, jac_stride, 0u, &nothing, &path);
  if (st0 || nothing) return st0;
  DeviceGuard guard(s->device);
  if (!guard.ok()) return INTERPN_HIP_ERR_NO_DEVICE;
  const size_t elem = s->dtype == kF64 ? 8 : 4;
  const size_t nd = (size_t)s->ndims, k = s->nfields, kn = k * nd;
  const long long opt_chunk = s->sub[0]->desc.cfg.host_chunk;
  size_t chunk = opt_chunk >= 1 ? (size_t)opt_chunk : ((size_t)2 << 20);
  if (chunk > npoints) chunk = npoints;
  // wide records or many fields would make a chunk large: its rows and its Jacobian rows within 256 MiB each
  const size_t widest = point_stride > kn ? point_stride : kn;
  const size_t cap = ((size_t)256 << 20) / (widest * elem);
  if (chunk > cap) chunk = cap ? cap : 1;
  std::lock_guard<std::mutex> host_lock(s->host_mu);
  if (!s->stream) HIP_TRY(pool_take_kit(s->device, &s->stream, &s->kit_word));
  const size_t rows_bytes = align_up(chunk * point_stride * elem, 256);
  const size_t vals_bytes = align_up(chunk * k * elem, 256);
  void* block = nullptr;  // the chunk's rows, then its packed value rows, then its packed Jacobian rows
  if (pool_alloc(s->device, &block, rows_bytes + vals_bytes + chunk * kn * elem) != hipSuccess) {
    (void)hipGetLastError();
    return INTERPN_HIP_ERR_OUT_OF_MEMORY;
  }
  char* values = static_cast<char*>(block) + rows_bytes;
  char* comps = values + vals_bytes;
  hipError_t err = hipSuccess;
  int st = INTERPN_HIP_OK;
  for (size_t begin = 0; begin < npoints && err == hipSuccess && st == INTERPN_HIP_OK; begin += chunk) {
    const size_t count = npoints - begin < chunk ? npoints - begin : chunk;
    // one copy of the interleaved rows; the last row ends with its last coordinate
    err = hipMemcpyAsync(block, static_cast<const char*>(pts) + begin * point_stride * elem, ((count - 1) * point_stride + nd) * elem,
                         hipMemcpyHostToDevice, s->stream);
    if (err != hipSuccess) break;
    st = points_grad_device(s, path, block, point_stride, count, values, k, comps, kn, s->stream, 0u);
    if (st) break;
    uint64_t bad = 0;
    st = interpn_hip_fields_finish(s, s->stream, &bad);
    const bool failed = st == s->sub[0]->desc.unrep_status;
    if (st && !failed) break;
    // the reference stops at the first failing point: the rows in front of it are written, everything else is left as it
    // was — the caller's elements behind a row's first K and K * N too
    const size_t good = failed ? (size_t)bad : count;
    char* vdst = static_cast<char*>(out) + begin * out_stride * elem;
    char* jdst = static_cast<char*>(jac) + begin * jac_stride * elem;
    if (good && out_stride == k) err = hipMemcpyAsync(vdst, values, good * k * elem, hipMemcpyDeviceToHost, s->stream);
    else if (good) err = hipMemcpy2DAsync(vdst, out_stride * elem, values, k * elem, k * elem, good, hipMemcpyDeviceToHost, s->stream);
    if (good && err == hipSuccess) {
      if (jac_stride == kn) err = hipMemcpyAsync(jdst, comps, good * kn * elem, hipMemcpyDeviceToHost, s->stream);
      else err = hipMemcpy2DAsync(jdst, jac_stride * elem, comps, kn * elem, kn * elem, good, hipMemcpyDeviceToHost, s->stream);
    }
    if (err == hipSuccess) err = hipStreamSynchronize(s->stream);
  }
  (void)hipStreamSynchronize(s->stream);  // nothing in flight touches the block when it goes back to the pool
  pool_free(s->device, block);
  if (err != hipSuccess) return hip_fail(err);
  return st;
}

}  // extern "C"
