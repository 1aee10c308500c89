// Field-set gradients on a lattice (include/interpn_hip.h, "Field-set gradients on a lattice"; lattice.h): path choice, the
// fused path (one axes launch and one launch of k_lattice_fields_grad_rows for all K fields), the per-field path (K
// lattice-gradient evaluations through the K handles, joined for fields-last results), the device- and host-pointer entry
// points, the reserve call and the plan.
// (C ABI internals, see abi_internal.h.)
#include "abi_internal.h"
#include "lattice.h"

using namespace interpn;
using namespace interpn_abi;

namespace {

using Slot = interpn_hip_interp::BinSlot;

constexpr size_t kHostChunkResultsFieldsLatticeGrad = (size_t)1 << 25;  // host form: results (points x K (N + 1)) per chunk

bool layout_ok(int layout) { return layout == INTERPN_HIP_FIELDS_LATTICE_FIELD_MAJOR || layout == INTERPN_HIP_FIELDS_LATTICE_FIELDS_LAST; }

FieldsLatticePlan plan_for(const interpn_hip_fields* s, const LatticeShape& sh, int layout) {
  const GridDesc& g = s->sub[0]->desc;  // the grid, the flavour and the options ("lattice", "axis_lds_kb") of every field
  if (!fast_path(g) || g.cfg.force_generic) return FieldsLatticePlan();  // 64-bit grids and the testing route: the handles' own kernels
  return fields_lattice_grad_plan(g.method, g.ndims, g.dtype == kF64 ? 8 : 4, g.n, sh.m, s->nfields, layout, lattice_lds_budget(g.cfg),
                                  g.cfg.num_cus, g.cfg.lattice);
}

// Whether a single handle's lattice-gradient call on `sh` runs its row kernel (abi_lattice_grad.hip's rule): it then needs
// none of the handle's re-laid tables.
bool single_fused(const GridDesc& g, const LatticeShape& sh) {
  if (!fast_path(g) || g.cfg.force_generic) return false;
  return lattice_grad_plan(g.method, g.ndims, g.dtype == kF64 ? 8 : 4, g.n, sh.m, lattice_lds_budget(g.cfg), g.cfg.num_cus, g.cfg.lattice)
      .fused;
}

// The per-field path's fields-last form works in slices of whole leading-axis indices: K (N + 1) scratch rows of a slice's
// points within kExpandSliceBytes together (option "points_slice" for tests), one leading index at least.
size_t slice_leading(const interpn_hip_fields* s, const LatticeShape& sh) {
  const size_t elem = s->dtype == kF64 ? 8 : 4;
  size_t points = kExpandSliceBytes / (s->nfields * (size_t)(s->ndims + 1) * elem);
  const long long opt = s->sub[0]->desc.cfg.points_slice;
  if (opt > 0) points = (size_t)opt;
  size_t lead = points / (size_t)sh.weight[0];
  if (lead < 1) lead = 1;
  return lead < sh.m[0] ? lead : sh.m[0];
}

size_t join_head(const interpn_hip_fields* s) { return align_up(s->nfields * sizeof(unsigned long long), 256); }

// Bytes of the first handle's block that holds the parked status words and the K (N + 1) rows of a slice.
size_t join_need(const interpn_hip_fields* s, const LatticeShape& sh) {
  const size_t elem = s->dtype == kF64 ? 8 : 4;
  return join_head(s) + s->nfields * (size_t)(s->ndims + 1) * align_up(slice_leading(s, sh) * (size_t)sh.weight[0] * elem, 256);
}

// One records block of the first handle, one axes launch, one rows launch: first-bad goes to the first handle's word.
int fused_device(interpn_hip_fields* s, const LatticeShape& sh, const FieldsLatticePlan& plan, void* out, size_t out_stride, void* jac,
                 size_t jac_stride, int layout, hipStream_t stream, unsigned flags) {
  interpn_hip_interp* h0 = s->sub[0];
  const GridDesc& g = h0->desc;
  const size_t elem = s->dtype == kF64 ? 8 : 4;
  const bool capturing = stream_capturing(stream);
  const size_t need = align_up(sh.coords * lattice_record_bytes(g.method, g.kind, elem), 256);
  int why = INTERPN_HIP_WHY_NONE;
  Slot* slot = capturing ? take_slot_captured(h0, need, stream) : take_bin_slot(h0, need, stream, !(flags & INTERPN_HIP_EVAL_NO_ALLOC), &why);
  if (!slot) return INTERPN_HIP_ERR_OUT_OF_MEMORY;  // no block reserved (interpn_hip_fields_reserve_lattice_grad) and none may be made
  claim_slot(h0, slot);
  hipError_t err = launch_lattice_axes(g, sh, slot->scratch, nullptr, h0->first_bad, stream);
  if (err == hipSuccess)
    err = launch_lattice_fields_grad_rows(g, sh, slot->scratch, s->field_stride, s->nfields, plan.group, out, out_stride, jac, jac_stride,
                                          layout, plan.lds_bytes, stream);
  if (capturing) release_slot_captured(h0, slot);
  else release_bin_slot(h0, slot, stream, false);
  if (err != hipSuccess) return fail_sequence(h0, err, INTERPN_HIP_OK);
  mark_stream(h0, stream);
  s->last_lattice_group = (int)plan.group;
  return INTERPN_HIP_OK;
}

// K lattice-gradient evaluations through the K handles, each with the handle's own paths.  Field-major results go straight
// into the caller's rows: grad[d] = jac + (f * N + d) * jac_stride.  Fields-last results: per slice of leading-axis indices
// (a lattice of its own) the K evaluations write K value rows and K N component rows of scratch, which two k_join_fields
// launches interleave into the caller's `out` and `jac` rows; the status words are parked around every slice but the
// first, as the value form's per_field_device (abi_fields_lattice.hip) does.
int per_field_device(interpn_hip_fields* s, const LatticeShape& sh, void* out, size_t out_stride, void* jac, size_t jac_stride,
                     int layout, hipStream_t stream, unsigned flags) {
  interpn_hip_interp* h0 = s->sub[0];
  const size_t elem = s->dtype == kF64 ? 8 : 4;
  const size_t k = s->nfields, nd = (size_t)s->ndims;
  const bool capturing = stream_capturing(stream);
  // evaluations that expand go through the handles' own kernels: their tables, once, where this call may build them
  const bool may_build = !(flags & INTERPN_HIP_EVAL_NO_ALLOC) && !capturing;
  auto tables_for = [&](const LatticeShape& shape) {
    if (s->sub_tables || !may_build || single_fused(h0->desc, shape)) return (int)INTERPN_HIP_OK;
    return ensure_sub_tables(s);
  };
  s->per_field_pending = true;
  if (layout == INTERPN_HIP_FIELDS_LATTICE_FIELD_MAJOR) {
    const int st0 = tables_for(sh);
    if (st0) return st0;
    for (size_t f = 0; f < k; ++f) {
      void* grad[8] = {nullptr};
      for (size_t d = 0; d < nd; ++d) grad[d] = static_cast<char*>(jac) + (f * nd + d) * jac_stride * elem;
      const int st = lattice_grad_device(s->sub[f], sh, static_cast<char*>(out) + f * out_stride * elem, grad, stream, flags, nullptr);
      if (st) return st;
    }
    return INTERPN_HIP_OK;
  }
  const size_t need = join_need(s, sh);
  int why = INTERPN_HIP_WHY_NONE;
  Slot* slot = capturing ? take_slot_captured(h0, need, stream) : take_bin_slot(h0, need, stream, !(flags & INTERPN_HIP_EVAL_NO_ALLOC), &why);
  if (!slot) return INTERPN_HIP_ERR_OUT_OF_MEMORY;  // no block reserved (interpn_hip_fields_reserve_lattice_grad) and none may be made
  claim_slot(h0, slot);
  unsigned char* scratch = static_cast<unsigned char*>(slot->scratch);
  unsigned long long* saved = reinterpret_cast<unsigned long long*>(scratch);
  const size_t per0 = (size_t)sh.weight[0];
  const size_t lead = slice_leading(s, sh);
  const size_t pitch = align_up(lead * per0 * elem, 256);
  unsigned char* vrows = scratch + join_head(s);  // K value rows, then K * N component rows (row f * N + d)
  unsigned char* grows = vrows + k * pitch;
  hipError_t err = hipSuccess;
  int st = INTERPN_HIP_OK;
  for (size_t i0 = 0; i0 < sh.m[0] && err == hipSuccess && st == INTERPN_HIP_OK; i0 += lead) {
    const size_t cnt0 = sh.m[0] - i0 < lead ? sh.m[0] - i0 : lead;
    const void* sub_axes[8];
    size_t sub_lens[8];
    for (int d = 0; d < sh.ndims; ++d) {
      sub_axes[d] = static_cast<const char*>(sh.axes[d]) + (d == 0 ? i0 * elem : 0);
      sub_lens[d] = d == 0 ? cnt0 : sh.m[d];
    }
    LatticeShape sub;
    st = lattice_make_shape(sub_axes, sub_lens, (size_t)sh.ndims, &sub);
    if (st == INTERPN_HIP_OK) st = tables_for(sub);
    if (st) break;
    const size_t words = i0 ? k : 0;
    for (size_t f = 0; f < words && err == hipSuccess; ++f) err = launch_points_bad_begin(s->sub[f]->first_bad, saved + f, stream);
    if (err != hipSuccess) break;  // (a word parked without its counterpart: the sequence failed as a whole)
    for (size_t f = 0; f < k && st == INTERPN_HIP_OK; ++f) {
      void* grad[8] = {nullptr};
      for (size_t d = 0; d < nd; ++d) grad[d] = grows + (f * nd + d) * pitch;
      st = lattice_grad_device(s->sub[f], sub, vrows + f * pitch, grad, stream, flags, nullptr);
    }
    for (size_t f = 0; f < words; ++f) {  // also behind a failed slice: the parked words go back
      const hipError_t e2 = launch_points_bad_end(s->sub[f]->first_bad, saved + f, (unsigned long long)(i0 * per0), stream);
      if (err == hipSuccess) err = e2;
    }
    if (err == hipSuccess && st == INTERPN_HIP_OK)
      err = launch_join_fields(h0->desc, vrows, pitch / elem, k, static_cast<char*>(out) + i0 * per0 * out_stride * elem, out_stride,
                               cnt0 * per0, stream);
    if (err == hipSuccess && st == INTERPN_HIP_OK)
      err = launch_join_fields(h0->desc, grows, pitch / elem, k * nd, static_cast<char*>(jac) + i0 * per0 * jac_stride * elem, jac_stride,
                               cnt0 * per0, stream);
  }
  if (capturing) release_slot_captured(h0, slot);
  else release_bin_slot(h0, slot, stream, false);
  if (err != hipSuccess || st != INTERPN_HIP_OK) return fail_sequence(h0, err, st);
  mark_stream(h0, stream);
  return INTERPN_HIP_OK;
}

// One lattice on device arrays.  Arguments are validated; the current device is the set's.
int fields_lattice_grad_device(interpn_hip_fields* s, const LatticeShape& sh, void* out, size_t out_stride, void* jac, size_t jac_stride,
                               int layout, hipStream_t stream, unsigned flags, int* path_taken) {
  const FieldsLatticePlan plan = plan_for(s, sh, layout);
  const int st = plan.fused ? fused_device(s, sh, plan, out, out_stride, jac, jac_stride, layout, stream, flags)
                            : per_field_device(s, sh, out, out_stride, jac, jac_stride, layout, stream, flags);
  if (st) return st;
  const int path = plan.fused ? INTERPN_HIP_FIELDS_LATTICE_PATH_FUSED : INTERPN_HIP_FIELDS_LATTICE_PATH_PER_FIELD;
  s->last_lattice_path = path;
  if (path_taken) *path_taken = path;
  return INTERPN_HIP_OK;
}

// What both entry points check, in this order: the set; validate_lattice on the first field's handle (its statuses; *empty:
// nothing to do); a nearest set; then `jac`, the layout value, the strides and the results' bytes.
int checks(const interpn_hip_fields* s, const void* const* axes, const size_t* axis_lens, size_t naxes, const void* out, size_t out_stride,
           const void* jac, size_t jac_stride, int layout, LatticeShape* sh, bool* empty) {
  *empty = false;
  if (!s || s->sub.empty()) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  const int st = validate_lattice(s->sub[0], axes, axis_lens, naxes, out, sh, empty);
  if (st || *empty) return st;
  const int method = s->sub[0]->desc.method;
  if (method != kLinear && method != kCubic) return INTERPN_HIP_ERR_UNSUPPORTED;  // nearest: no gradient form
  if (!jac || !layout_ok(layout)) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  const size_t k = s->nfields, nd = (size_t)s->ndims;
  const bool major = layout == INTERPN_HIP_FIELDS_LATTICE_FIELD_MAJOR;
  if (major ? (out_stride < sh->npoints || jac_stride < sh->npoints) : (out_stride < k || jac_stride < k * nd))
    return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  size_t total = 0;  // both results' bytes fit size_t
  if (__builtin_mul_overflow(major ? k : sh->npoints, out_stride, &total) || total > (~(size_t)0) / 8) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  if (__builtin_mul_overflow(major ? k * nd : sh->npoints, jac_stride, &total) || total > (~(size_t)0) / 8)
    return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  return INTERPN_HIP_OK;
}

}  // namespace

extern "C" {

int interpn_hip_fields_eval_lattice_grad_device(interpn_hip_fields* s, const void* const* axes, const size_t* axis_lens, size_t naxes,
                                                void* out, size_t out_stride, void* jac, size_t jac_stride, int layout, void* stream,
                                                unsigned flags, int* path_taken) {
  if (path_taken) *path_taken = INTERPN_HIP_FIELDS_LATTICE_PATH_PER_FIELD;
  if (flags & ~(unsigned)INTERPN_HIP_EVAL_NO_ALLOC) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  LatticeShape sh;
  bool empty = false;
  const int st = checks(s, axes, axis_lens, naxes, out, out_stride, jac, jac_stride, layout, &sh, &empty);
  if (st || empty) return st;
  DeviceGuard guard(s->device);
  if (!guard.ok()) return INTERPN_HIP_ERR_NO_DEVICE;
  return fields_lattice_grad_device(s, sh, out, out_stride, jac, jac_stride, layout, static_cast<hipStream_t>(stream), flags, path_taken);
}

int interpn_hip_fields_reserve_lattice_grad(interpn_hip_fields* s, const size_t* axis_lens, size_t naxes, int nstreams) {
  if (!s || s->sub.empty() || nstreams < 0 || (!axis_lens && naxes)) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  interpn_hip_interp* h0 = s->sub[0];
  if (is_one_dim(h0->desc.method)) return INTERPN_HIP_ERR_UNSUPPORTED;
  int st = validate_obs(h0->desc, nullptr, naxes, 0);
  if (st) return st;
  LatticeShape sh;
  st = lattice_make_shape(nullptr, axis_lens, naxes, &sh);
  if (st) return st;
  if (h0->desc.method != kLinear && h0->desc.method != kCubic) return INTERPN_HIP_ERR_UNSUPPORTED;  // nearest: no gradient form
  if ((size_t)nstreams > interpn_hip_interp::kMaxBinSlots) nstreams = (int)interpn_hip_interp::kMaxBinSlots;
  if (sh.npoints == 0 || nstreams == 0) return INTERPN_HIP_OK;
  DeviceGuard guard(s->device);
  if (!guard.ok()) return INTERPN_HIP_ERR_NO_DEVICE;
  // what interpn_hip_fields_reserve_lattice does (a single handle's gradient call takes the value call's scratch), with the
  // per-field slice sized for K (N + 1) rows; the same two-stream limit for the fields-last per-field form
  for (size_t f = 1; f < s->nfields; ++f) {
    st = reserve_slots(s->sub[f], lattice_reserve_need(s->sub[f]->desc, sh), nstreams);
    if (st) return st;
  }
  size_t need = lattice_reserve_need(h0->desc, sh);
  const size_t rows = join_need(s, sh);
  if (rows > need) need = rows;
  int blocks = 2 * nstreams;
  if ((size_t)blocks > interpn_hip_interp::kMaxBinSlots) blocks = (int)interpn_hip_interp::kMaxBinSlots;
  return reserve_slots(h0, need, blocks);
}

int interpn_hip_fields_eval_lattice_grad_host(interpn_hip_fields* s, const void* const* axes, const size_t* axis_lens, size_t naxes,
                                              void* out, size_t out_stride, void* jac, size_t jac_stride, int layout,
                                              uint64_t* first_bad_index) {
  LatticeShape sh;
  bool empty = false;
  int st = checks(s, axes, axis_lens, naxes, out, out_stride, jac, jac_stride, layout, &sh, &empty);
  if (st || empty) return st;
  DeviceGuard guard(s->device);
  if (!guard.ok()) return INTERPN_HIP_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> host_lock(s->host_mu);
  if (!s->stream) HIP_TRY(pool_take_kit(s->device, &s->stream, &s->kit_word));
  const size_t elem = s->dtype == kF64 ? 8 : 4;
  const size_t k = s->nfields, nd = (size_t)s->ndims, kn = k * nd;
  const bool last = layout == INTERPN_HIP_FIELDS_LATTICE_FIELDS_LAST;
  // Chunks of leading-axis indices, each a lattice of its own: about 2^25 / (K (N + 1)) points (option "host_chunk": points)
  const size_t per0 = (size_t)sh.weight[0];
  const long long opt_chunk = s->sub[0]->desc.cfg.host_chunk;
  const size_t chunk_points = opt_chunk >= 1 ? (size_t)opt_chunk : kHostChunkResultsFieldsLatticeGrad / (k * (nd + 1));
  size_t rows0 = chunk_points / per0;
  if (rows0 < 1) rows0 = 1;
  if (rows0 > sh.m[0]) rows0 = sh.m[0];
  // one block: every axis (each 256-byte aligned), then the chunk's values and its Jacobian in the caller's layout, packed
  size_t axes_bytes = 0, off[8] = {0};
  for (int d = 0; d < sh.ndims; ++d) { off[d] = axes_bytes; axes_bytes += align_up(sh.m[d] * elem, 256); }
  const size_t out_bytes = align_up(rows0 * per0 * k * elem, 256);
  void* block = nullptr;
  if (pool_alloc(s->device, &block, axes_bytes + out_bytes + rows0 * per0 * kn * elem) != hipSuccess) { (void)hipGetLastError(); return INTERPN_HIP_ERR_OUT_OF_MEMORY; }
  char* dev_out = static_cast<char*>(block) + axes_bytes;
  char* dev_jac = dev_out + out_bytes;
  hipError_t err = hipSuccess;
  for (int d = 0; d < sh.ndims && err == hipSuccess; ++d)
    err = hipMemcpyAsync(static_cast<char*>(block) + off[d], axes[d], sh.m[d] * elem, hipMemcpyHostToDevice, s->stream);
  st = INTERPN_HIP_OK;
  for (size_t i0 = 0; i0 < sh.m[0] && err == hipSuccess && st == INTERPN_HIP_OK; i0 += rows0) {
    const size_t cnt0 = sh.m[0] - i0 < rows0 ? sh.m[0] - i0 : rows0;
    const void* sub_axes[8];
    size_t sub_lens[8];
    for (int d = 0; d < sh.ndims; ++d) {
      sub_axes[d] = static_cast<char*>(block) + off[d] + (d == 0 ? i0 * elem : 0);
      sub_lens[d] = d == 0 ? cnt0 : sh.m[d];
    }
    LatticeShape sub;
    st = lattice_make_shape(sub_axes, sub_lens, (size_t)sh.ndims, &sub);
    if (st) break;
    const size_t count = sub.npoints;
    st = fields_lattice_grad_device(s, sub, dev_out, last ? k : count, dev_jac, last ? kn : count, layout, s->stream, 0u, nullptr);
    if (st) break;
    uint64_t bad = 0;
    st = interpn_hip_fields_finish(s, s->stream, &bad);
    const bool failed = st == s->sub[0]->desc.unrep_status;
    if (st && !failed) break;
    // the reference's loop stops at the first failing point: the results in front of it are written — of every field and
    // every component — and everything else is left as it was, the caller's padding columns too
    const size_t good = failed ? (size_t)bad : count;
    if (failed && first_bad_index) *first_bad_index = (uint64_t)(i0 * per0 + good);
    if (good && !last) {
      for (size_t f = 0; f < k && err == hipSuccess; ++f)
        err = hipMemcpyAsync(static_cast<char*>(out) + (f * out_stride + i0 * per0) * elem, dev_out + f * count * elem, good * elem,
                             hipMemcpyDeviceToHost, s->stream);
      for (size_t r = 0; r < kn && err == hipSuccess; ++r)
        err = hipMemcpyAsync(static_cast<char*>(jac) + (r * jac_stride + i0 * per0) * elem, dev_jac + r * count * elem, good * elem,
                             hipMemcpyDeviceToHost, s->stream);
    } else if (good) {
      char* dst = static_cast<char*>(out) + i0 * per0 * out_stride * elem;
      if (out_stride == k) err = hipMemcpyAsync(dst, dev_out, good * k * elem, hipMemcpyDeviceToHost, s->stream);
      else err = hipMemcpy2DAsync(dst, out_stride * elem, dev_out, k * elem, k * elem, good, hipMemcpyDeviceToHost, s->stream);
      char* dstj = static_cast<char*>(jac) + i0 * per0 * jac_stride * elem;
      if (err == hipSuccess && jac_stride == kn) err = hipMemcpyAsync(dstj, dev_jac, good * kn * elem, hipMemcpyDeviceToHost, s->stream);
      else if (err == hipSuccess)
        err = hipMemcpy2DAsync(dstj, jac_stride * elem, dev_jac, kn * elem, kn * elem, good, hipMemcpyDeviceToHost, s->stream);
    }
    if (err == hipSuccess) err = hipStreamSynchronize(s->stream);
  }
  (void)hipStreamSynchronize(s->stream);  // nothing in flight touches the block when it goes back to the pool
  pool_free(s->device, block);
  if (err != hipSuccess) return hip_fail(err);
  return st;
}

int interpn_hip_fields_lattice_grad_plan(size_t elem_size, int method, size_t ndims, const size_t* dims, const size_t* axis_lens,
                                         size_t nfields, int layout, int* path, size_t* group, size_t* lds_bytes, size_t* npoints) {
  int n[8] = {0};
  LatticeShape sh;
  bool indexable = false;
  const int st = lattice_plan_args(elem_size, method, ndims, dims, axis_lens, n, &sh, &indexable);
  if (st) return st;
  method &= 0xFF;
  if (method == kNearest) return INTERPN_HIP_ERR_UNSUPPORTED;  // no gradient form
  if (nfields == 0 || !layout_ok(layout)) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  LaunchConfig c;  // the defaults of a handle on an MI355X, with the environment a new handle would latch
  latch_env(c);
  FieldsLatticePlan p;
  if (indexable && sh.npoints && !c.force_generic)
    p = fields_lattice_grad_plan(method, (int)ndims, elem_size, n, sh.m, nfields, layout, lattice_lds_budget(c), c.num_cus, c.lattice);
  if (path) *path = p.fused ? INTERPN_HIP_FIELDS_LATTICE_PATH_FUSED : INTERPN_HIP_FIELDS_LATTICE_PATH_PER_FIELD;
  if (group) *group = p.group;
  if (lds_bytes) *lds_bytes = p.lds_bytes;
  if (npoints) *npoints = sh.npoints;
  return INTERPN_HIP_OK;
}

}  // extern "C"
