// Lattice evaluation (lattice.h): path choice, scratch, the device- and host-pointer entry points.
// (C ABI internals, see abi_internal.h.)
#include "abi_internal.h"
#include "lattice.h"

using namespace interpn;
using namespace interpn_abi;

namespace interpn_abi {

using Slot = interpn_hip_interp::BinSlot;

// Under graph capture no event of a block may be queried, waited for or recorded: scratch_slots.h takes a block without.
Slot* take_slot_captured(interpn_hip_interp* h, size_t need, hipStream_t stream) { return scratch_slots::take_slot_captured(*h, need, stream); }

void release_slot_captured(interpn_hip_interp* h, Slot* slot) { scratch_slots::release_slot_captured(*h, slot); }

// The block's contents are the caller's now: the sort's and the sweep's invariants about it are gone.
void claim_slot(interpn_hip_interp* h, Slot* slot) {
  std::lock_guard<std::mutex> lk(h->bin_mu);
  slot->totals_clean = false;
  slot->sweep_clean = false;
  slot->staged = false;
  const unsigned char* word = static_cast<const unsigned char*>(h->sampling.last_word);
  const unsigned char* base = static_cast<const unsigned char*>(slot->scratch);
  if (word && word >= base && word < base + slot->bytes) h->sampling.last_word = nullptr;
}

// `nstreams` blocks of at least `need` bytes (scratch_slots.h: reserve_blocks; also what interpn_hip_reserve ends in).
int reserve_slots(interpn_hip_interp* h, size_t need, int nstreams) {
  int rt_error = 0;
  const int st = scratch_slots::reserve_blocks(*h, need, nstreams, &rt_error);
  return st < 0 ? hip_fail((hipError_t)rt_error) : st;
}

}  // namespace interpn_abi

namespace {

constexpr size_t kHostChunkPointsLattice = (size_t)1 << 25;  // host form: lattice points per chunk of leading-axis indices

}  // namespace

namespace interpn_abi {

// Shape of a lattice from the caller's arrays.  INVALID_ARGUMENT: the point count does not fit size_t;
// UNSUPPORTED: more than 2^31 axis coordinates in all.
int lattice_make_shape(const void* const* axes, const size_t* axis_lens, size_t naxes, LatticeShape* s) {
  s->ndims = (int)naxes;
  size_t np = 0;
  if (!checked_product(axis_lens, naxes, &np)) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  s->npoints = np;
  size_t coords = 0;
  for (size_t d = 0; d < naxes; ++d) {
    s->axes[d] = axes ? axes[d] : nullptr;
    s->m[d] = axis_lens[d];
    if (coords > kLatticeMaxCoords || axis_lens[d] > kLatticeMaxCoords) return INTERPN_HIP_ERR_UNSUPPORTED;
    s->rec_off[d] = (unsigned)coords;
    coords += axis_lens[d];
  }
  if (coords > kLatticeMaxCoords) return INTERPN_HIP_ERR_UNSUPPORTED;
  s->coords = coords;
  unsigned long long w = 1;
  for (int d = (int)naxes - 1; d >= 0; --d) {
    s->weight[d] = w;
    w *= (unsigned long long)(axis_lens[d] ? axis_lens[d] : 1);  // (npoints fits size_t: so does every partial product of non-zero lengths)
  }
  return INTERPN_HIP_OK;
}

LatticePlan lattice_plan_for(const GridDesc& g, const LatticeShape& s) {
  if (!fast_path(g) || g.cfg.force_generic) return LatticePlan();  // 64-bit grids and the testing route: the handle's own kernels
  return lattice_plan(g.method, g.ndims, g.dtype == kF64 ? 8 : 4, g.n, s.m, lattice_lds_budget(g.cfg), g.cfg.num_cus, g.cfg.lattice);
}

// Points per slice of the expanded path.
size_t lattice_expand_slice(const GridDesc& g, size_t npoints) {
  const size_t elem = g.dtype == kF64 ? 8 : 4;
  size_t slice = kExpandSliceBytes / ((size_t)g.ndims * elem);
  if (slice < kExpandSliceMin) slice = kExpandSliceMin;
  slice &= ~(size_t)255;  // slices begin 16-byte aligned in `out` and in the coordinate arrays (sweep evaluation)
  return npoints < slice ? npoints : slice;
}

// Bytes of the scratch block one evaluation needs.
size_t lattice_scratch_need(const GridDesc& g, const LatticeShape& s, const LatticePlan& p) {
  const size_t elem = g.dtype == kF64 ? 8 : 4;
  if (p.fused) return align_up(s.coords * lattice_record_bytes(g.method, g.kind, elem), 256);
  const size_t flags = g.kind == kRegular ? align_up(s.coords, 256) : 0;
  return flags + (size_t)g.ndims * align_up(lattice_expand_slice(g, s.npoints) * elem, 256);
}

// One lattice on device arrays.  Arguments are validated; the current device is the handle's.
int lattice_device(interpn_hip_interp* h, const LatticeShape& s, void* out, hipStream_t stream, unsigned flags, int* path_taken) {
  const GridDesc& g = h->desc;
  const LatticePlan plan = lattice_plan_for(g, s);
  const size_t elem = g.dtype == kF64 ? 8 : 4;
  const bool capturing = stream_capturing(stream);
  const size_t need = lattice_scratch_need(g, s, plan);
  Slot* slot = nullptr;
  if (need) {
    int why = INTERPN_HIP_WHY_NONE;
    slot = capturing ? take_slot_captured(h, need, stream)
                     : take_bin_slot(h, need, stream, !(flags & INTERPN_HIP_EVAL_NO_ALLOC), &why);
    if (!slot) return INTERPN_HIP_ERR_OUT_OF_MEMORY;  // no block reserved (interpn_hip_reserve_lattice) and none may be made
    claim_slot(h, slot);
  }
  unsigned char* scratch = slot ? static_cast<unsigned char*>(slot->scratch) : nullptr;
  hipError_t err = hipSuccess;
  int st = INTERPN_HIP_OK;
  if (plan.fused) {
    err = launch_lattice_axes(g, s, scratch, nullptr, h->first_bad, stream);
    if (err == hipSuccess) err = launch_lattice_rows(g, s, scratch, out, plan.lds_bytes, stream);
  } else {
    unsigned char* bad = g.kind == kRegular ? scratch : nullptr;
    const size_t flags_bytes = bad ? align_up(s.coords, 256) : 0;
    const size_t slice = lattice_expand_slice(g, s.npoints);
    const size_t pitch = align_up(slice * elem, 256);
    void* dst[8] = {nullptr};
    for (int d = 0; d < g.ndims; ++d) dst[d] = scratch + flags_bytes + (size_t)d * pitch;
    err = launch_lattice_axes(g, s, nullptr, bad, h->first_bad, stream);
    for (size_t begin = 0; begin < s.npoints && err == hipSuccess && st == INTERPN_HIP_OK; begin += slice) {
      const size_t count = s.npoints - begin < slice ? s.npoints - begin : slice;
      err = launch_lattice_expand(g, s, bad, dst, begin, count, stream);
      if (err != hipSuccess) break;
      st = interpn_hip_eval_device_ex(h, dst, (size_t)g.ndims, static_cast<char*>(out) + begin * elem, count, stream,
                                      flags & INTERPN_HIP_EVAL_NO_ALLOC, nullptr, nullptr);
    }
  }
  if (slot) {
    if (capturing) release_slot_captured(h, slot);
    else release_bin_slot(h, slot, stream, false);
  }
  if (err != hipSuccess || st != INTERPN_HIP_OK) return fail_sequence(h, err, st);
  const int path = plan.fused ? INTERPN_HIP_LATTICE_PATH_FUSED : INTERPN_HIP_LATTICE_PATH_EXPANDED;
  h->desc.last_lattice_path = path;
  if (path_taken) *path_taken = path;
  mark_stream(h, stream);
  return INTERPN_HIP_OK;
}

// What every lattice entry point checks, in this order; *empty: some axis has no coordinates (nothing to do).
int validate_lattice(const interpn_hip_interp* h, const void* const* axes, const size_t* axis_lens, size_t naxes, const void* out,
                     LatticeShape* s, bool* empty) {
  if (!h || (!axes && naxes) || (!axis_lens && naxes)) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  if (is_one_dim(h->desc.method)) return INTERPN_HIP_ERR_UNSUPPORTED;
  int st = validate_obs(h->desc, nullptr, naxes, 0);
  if (st) return st;
  st = lattice_make_shape(axes, axis_lens, naxes, s);
  if (st) return st;
  *empty = s->npoints == 0;
  if (*empty) return INTERPN_HIP_OK;
  if (!out) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  for (size_t d = 0; d < naxes; ++d)
    if (!axes[d]) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  return INTERPN_HIP_OK;
}

// What interpn_hip_lattice_plan and interpn_hip_fields_lattice_plan check, in this order.
int lattice_plan_args(size_t elem_size, int method, size_t ndims, const size_t* dims, const size_t* axis_lens, int* n, LatticeShape* s,
                      bool* indexable) {
  method &= 0xFF;
  if ((elem_size != 4 && elem_size != 8) || (method != kLinear && method != kCubic && method != kNearest)) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  if (ndims < 1 || ndims > 8 || !dims || !axis_lens) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  const size_t minlen = method == kCubic ? 4 : 2;
  const size_t maxlen = elem_size == 8 ? max_axis_len<double>() : max_axis_len<float>();
  for (size_t d = 0; d < ndims; ++d) {
    if (dims[d] < minlen) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
    if (dims[d] > maxlen) return INTERPN_HIP_ERR_UNSUPPORTED;
    n[d] = (int)dims[d];
  }
  int st = lattice_make_shape(nullptr, axis_lens, ndims, s);
  if (st) return st;
  size_t nvals = 0;
  *indexable = checked_product(dims, ndims, &nvals) && nvals < 0xFFFFFFFFull;
  return INTERPN_HIP_OK;
}

// Whichever path the options in force at evaluation time choose: the larger of the two blocks.
size_t lattice_reserve_need(const GridDesc& g, const LatticeShape& s) {
  LatticePlan fused = lattice_plan_for(g, s), expanded;
  size_t need = lattice_scratch_need(g, s, expanded);
  if (fused.covered && fused.fits) {
    fused.fused = true;
    const size_t nf = lattice_scratch_need(g, s, fused);
    if (nf > need) need = nf;
  }
  return need;
}

}  // namespace interpn_abi

extern "C" {

int interpn_hip_lattice_plan(size_t elem_size, int method, size_t ndims, const size_t* dims, const size_t* axis_lens,
                             int* path, size_t* lds_bytes, size_t* npoints) {
  int n[8] = {0};
  LatticeShape s;
  bool indexable = false;
  const int st = lattice_plan_args(elem_size, method, ndims, dims, axis_lens, n, &s, &indexable);
  if (st) return st;
  method &= 0xFF;
  LaunchConfig c;  // the defaults of a handle on an MI355X, with the environment a new handle would latch
  latch_env(c);
  LatticePlan p;
  if (indexable && s.npoints && !c.force_generic)
    p = lattice_plan(method, (int)ndims, elem_size, n, s.m, lattice_lds_budget(c), c.num_cus, c.lattice);
  if (path) *path = p.fused ? INTERPN_HIP_LATTICE_PATH_FUSED : INTERPN_HIP_LATTICE_PATH_EXPANDED;
  if (lds_bytes) *lds_bytes = p.lds_bytes;
  if (npoints) *npoints = s.npoints;
  return INTERPN_HIP_OK;
}

int interpn_hip_eval_lattice_device(interpn_hip_interp* h, const void* const* axes, const size_t* axis_lens, size_t naxes,
                                    void* out, void* stream, unsigned flags, int* path_taken) {
  if (path_taken) *path_taken = INTERPN_HIP_LATTICE_PATH_EXPANDED;
  if (flags & ~(unsigned)INTERPN_HIP_EVAL_NO_ALLOC) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  LatticeShape s;
  bool empty = false;
  const int st = validate_lattice(h, axes, axis_lens, naxes, out, &s, &empty);
  if (st || empty) return st;
  DeviceGuard guard(h->device);
  if (!guard.ok()) return INTERPN_HIP_ERR_NO_DEVICE;
  return lattice_device(h, s, out, static_cast<hipStream_t>(stream), flags, path_taken);
}

int interpn_hip_reserve_lattice(interpn_hip_interp* h, const size_t* axis_lens, size_t naxes, int nstreams) {
  if (!h || nstreams < 0 || (!axis_lens && naxes)) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  if (is_one_dim(h->desc.method)) return INTERPN_HIP_ERR_UNSUPPORTED;
  int st = validate_obs(h->desc, nullptr, naxes, 0);
  if (st) return st;
  LatticeShape s;
  st = lattice_make_shape(nullptr, axis_lens, naxes, &s);
  if (st) return st;
  if ((size_t)nstreams > interpn_hip_interp::kMaxBinSlots) nstreams = (int)interpn_hip_interp::kMaxBinSlots;
  if (s.npoints == 0 || nstreams == 0) return INTERPN_HIP_OK;
  const GridDesc& g = h->desc;
  const size_t need = lattice_reserve_need(g, s);
  DeviceGuard guard(h->device);
  if (!guard.ok()) return INTERPN_HIP_ERR_NO_DEVICE;
  return reserve_slots(h, need, nstreams);
}

int interpn_hip_eval_lattice_host(interpn_hip_interp* h, const void* const* axes, const size_t* axis_lens, size_t naxes,
                                  void* out, uint64_t* first_bad_index) {
  LatticeShape s;
  bool empty = false;
  int st = validate_lattice(h, axes, axis_lens, naxes, out, &s, &empty);
  if (st || empty) return st;
  std::lock_guard<std::mutex> host_lock(h->host_mu);
  DeviceGuard guard(h->device);
  if (!guard.ok()) return INTERPN_HIP_ERR_NO_DEVICE;
  interpn_hip_interp::HostLane& l = h->lane[0];
  if (!l.stream) HIP_TRY(pool_take_kit(h->device, &l.stream, &l.flag_host));
  const size_t elem = h->desc.dtype == kF64 ? 8 : 4;
  // Chunks of leading-axis indices: each is a lattice of its own, so the device result of one chunk is bounded.
  const size_t per0 = (size_t)s.weight[0];
  size_t rows0 = kHostChunkPointsLattice / per0;
  if (rows0 < 1) rows0 = 1;
  if (rows0 > s.m[0]) rows0 = s.m[0];
  // one block: every axis (each 256-byte aligned), then the chunk's results
  size_t axes_bytes = 0, off[8] = {0};
  for (int d = 0; d < s.ndims; ++d) { off[d] = axes_bytes; axes_bytes += align_up(s.m[d] * elem, 256); }
  void* block = nullptr;
  HIP_TRY(pool_alloc(h->device, &block, axes_bytes + rows0 * per0 * elem));
  char* dev_out = static_cast<char*>(block) + axes_bytes;
  hipError_t err = hipSuccess;
  for (int d = 0; d < s.ndims && err == hipSuccess; ++d)
    err = hipMemcpyAsync(static_cast<char*>(block) + off[d], axes[d], s.m[d] * elem, hipMemcpyHostToDevice, l.stream);
  st = INTERPN_HIP_OK;
  for (size_t i0 = 0; i0 < s.m[0] && err == hipSuccess && st == INTERPN_HIP_OK; i0 += rows0) {
    const size_t cnt0 = s.m[0] - i0 < rows0 ? s.m[0] - i0 : rows0;
    const void* sub_axes[8];
    size_t sub_lens[8];
    for (int d = 0; d < s.ndims; ++d) {
      sub_axes[d] = static_cast<char*>(block) + off[d] + (d == 0 ? i0 * elem : 0);
      sub_lens[d] = d == 0 ? cnt0 : s.m[d];
    }
    LatticeShape sub;
    st = lattice_make_shape(sub_axes, sub_lens, (size_t)s.ndims, &sub);
    if (st) break;
    st = lattice_device(h, sub, dev_out, l.stream, 0u, nullptr);
    if (st) break;
    err = hipMemcpyAsync(l.flag_host, h->first_bad, sizeof(unsigned long long), hipMemcpyDeviceToHost, l.stream);
    if (err == hipSuccess) err = hipStreamSynchronize(l.stream);
    if (err != hipSuccess) break;
    const unsigned long long bad = *l.flag_host;
    size_t good = sub.npoints;
    if (bad != kNoBadIndexHost) {
      err = hipMemsetAsync(h->first_bad, 0xFF, sizeof(unsigned long long), l.stream);
      good = (size_t)bad;  // the reference's loop stops here: out[0 .. i) written, out[i ..] untouched
      if (first_bad_index) *first_bad_index = (uint64_t)(i0 * per0 + good);
      st = h->desc.unrep_status;
    }
    if (good && err == hipSuccess)
      err = hipMemcpyAsync(static_cast<char*>(out) + i0 * per0 * elem, dev_out, good * elem, hipMemcpyDeviceToHost, l.stream);
    if (err == hipSuccess) err = hipStreamSynchronize(l.stream);
  }
  (void)hipStreamSynchronize(l.stream);  // nothing in flight touches the block when it goes back to the pool
  pool_free(h->device, block);
  if (err != hipSuccess) return hip_fail(err);
  return st;
}

}  // extern "C"
