// Gradients on a lattice (include/interpn_hip.h, "Gradients on a lattice"; lattice.h, lattice_grad.h): path choice, the
// fused path (the axes launch of the value call and one launch of k_lattice_grad_rows), the expanded path (the value
// call's flags pass and slices, each slice through interpn_hip_eval_grad_device / interpn_hip_eval_cubic_grad_device), the
// device- and host-pointer entry points.  Scratch is the value call's, so interpn_hip_reserve_lattice serves both.
// (C ABI internals, see abi_internal.h.)
#include "abi_internal.h"
#include "lattice.h"

using namespace interpn;
using namespace interpn_abi;

namespace {

using Slot = interpn_hip_interp::BinSlot;

constexpr size_t kHostChunkResultsLatticeGrad = (size_t)1 << 25;  // host form: results (points x (N + 1)) per chunk of leading-axis indices

LatticePlan grad_plan_for(const GridDesc& g, const LatticeShape& s) {
  if (!fast_path(g) || g.cfg.force_generic) return LatticePlan();  // 64-bit grids and the testing route: the handle's own kernels
  return lattice_grad_plan(g.method, g.ndims, g.dtype == kF64 ? 8 : 4, g.n, s.m, lattice_lds_budget(g.cfg), g.cfg.num_cus, g.cfg.lattice);
}

}  // namespace

namespace interpn_abi {

// One lattice on device arrays.  Arguments are validated; the current device is the handle's.  (abi_internal.h: also the
// per-field path of a field set, abi_fields_lattice_grad.hip.)
int lattice_grad_device(interpn_hip_interp* h, const LatticeShape& s, void* out, void* const* grad, hipStream_t stream, unsigned flags,
                        int* path_taken) {
  const GridDesc& g = h->desc;
  const LatticePlan plan = grad_plan_for(g, s);
  const size_t elem = g.dtype == kF64 ? 8 : 4;
  const bool capturing = stream_capturing(stream);
  const size_t need = lattice_scratch_need(g, s, plan);  // records when fused, flags and a coordinate slice when not: the value call's
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
    if (err == hipSuccess) err = launch_lattice_grad_rows(g, s, scratch, out, grad, plan.lds_bytes, stream);
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
      void* gslice[8] = {nullptr};
      for (int d = 0; d < g.ndims; ++d) gslice[d] = static_cast<char*>(grad[d]) + begin * elem;
      void* oslice = static_cast<char*>(out) + begin * elem;
      st = g.method == kCubic ? interpn_hip_eval_cubic_grad_device(h, dst, (size_t)g.ndims, oslice, gslice, count, stream)
                              : interpn_hip_eval_grad_device(h, dst, (size_t)g.ndims, oslice, gslice, count, stream);
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

}  // namespace interpn_abi

namespace {

// validate_lattice's checks in their order, then the method, then the gradient arrays; *empty: nothing to do.
int checks(const interpn_hip_interp* h, const void* const* axes, const size_t* axis_lens, size_t naxes, const void* out,
           void* const* grad, LatticeShape* s, bool* empty) {
  *empty = false;
  const int st = validate_lattice(h, axes, axis_lens, naxes, out, s, empty);
  if (st) return st;
  if (h->desc.method != kLinear && h->desc.method != kCubic) return INTERPN_HIP_ERR_UNSUPPORTED;  // nearest: no gradient form
  if (*empty) return INTERPN_HIP_OK;
  if (!grad) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  for (size_t d = 0; d < naxes; ++d)
    if (!grad[d]) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  return INTERPN_HIP_OK;
}

}  // namespace

extern "C" {

int interpn_hip_lattice_grad_plan(size_t elem_size, int method, size_t ndims, const size_t* dims, const size_t* axis_lens,
                                  int* path, size_t* lds_bytes, size_t* npoints) {
  int n[8] = {0};
  LatticeShape s;
  bool indexable = false;
  const int st = lattice_plan_args(elem_size, method, ndims, dims, axis_lens, n, &s, &indexable);
  if (st) return st;
  method &= 0xFF;
  if (method == kNearest) return INTERPN_HIP_ERR_UNSUPPORTED;
  LaunchConfig c;  // the defaults of a handle on an MI355X, with the environment a new handle would latch
  latch_env(c);
  LatticePlan p;
  if (indexable && s.npoints && !c.force_generic)
    p = lattice_grad_plan(method, (int)ndims, elem_size, n, s.m, lattice_lds_budget(c), c.num_cus, c.lattice);
  if (path) *path = p.fused ? INTERPN_HIP_LATTICE_PATH_FUSED : INTERPN_HIP_LATTICE_PATH_EXPANDED;
  if (lds_bytes) *lds_bytes = p.lds_bytes;
  if (npoints) *npoints = s.npoints;
  return INTERPN_HIP_OK;
}

int interpn_hip_eval_lattice_grad_device(interpn_hip_interp* h, const void* const* axes, const size_t* axis_lens, size_t naxes,
                                         void* out, void* const* grad, void* stream, unsigned flags, int* path_taken) {
  if (path_taken) *path_taken = INTERPN_HIP_LATTICE_PATH_EXPANDED;
  if (flags & ~(unsigned)INTERPN_HIP_EVAL_NO_ALLOC) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  LatticeShape s;
  bool empty = false;
  const int st = checks(h, axes, axis_lens, naxes, out, grad, &s, &empty);
  if (st || empty) return st;
  DeviceGuard guard(h->device);
  if (!guard.ok()) return INTERPN_HIP_ERR_NO_DEVICE;
  return lattice_grad_device(h, s, out, grad, static_cast<hipStream_t>(stream), flags, path_taken);
}

int interpn_hip_eval_lattice_grad_host(interpn_hip_interp* h, const void* const* axes, const size_t* axis_lens, size_t naxes,
                                       void* out, void* const* grad, uint64_t* first_bad_index) {
  LatticeShape s;
  bool empty = false;
  int st = checks(h, axes, axis_lens, naxes, out, grad, &s, &empty);
  if (st || empty) return st;
  std::lock_guard<std::mutex> host_lock(h->host_mu);
  DeviceGuard guard(h->device);
  if (!guard.ok()) return INTERPN_HIP_ERR_NO_DEVICE;
  interpn_hip_interp::HostLane& l = h->lane[0];
  if (!l.stream) HIP_TRY(pool_take_kit(h->device, &l.stream, &l.flag_host));
  const size_t elem = h->desc.dtype == kF64 ? 8 : 4;
  const int nd = s.ndims;
  // Chunks of leading-axis indices, each a lattice of its own: about 2^25 / (N + 1) points (option "host_chunk": points)
  const size_t per0 = (size_t)s.weight[0];
  const long long opt_chunk = h->desc.cfg.host_chunk;
  const size_t chunk_points = opt_chunk >= 1 ? (size_t)opt_chunk : kHostChunkResultsLatticeGrad / (size_t)(nd + 1);
  size_t rows0 = chunk_points / per0;
  if (rows0 < 1) rows0 = 1;
  if (rows0 > s.m[0]) rows0 = s.m[0];
  // one block: every axis (each 256-byte aligned), then the chunk's values and its N component arrays
  size_t axes_bytes = 0, off[8] = {0};
  for (int d = 0; d < nd; ++d) { off[d] = axes_bytes; axes_bytes += align_up(s.m[d] * elem, 256); }
  const size_t pitch = align_up(rows0 * per0 * elem, 256);
  void* block = nullptr;
  if (pool_alloc(h->device, &block, axes_bytes + (size_t)(nd + 1) * pitch) != hipSuccess) { (void)hipGetLastError(); return INTERPN_HIP_ERR_OUT_OF_MEMORY; }
  char* dev_out = static_cast<char*>(block) + axes_bytes;
  void* dev_grad[8] = {nullptr};
  for (int d = 0; d < nd; ++d) dev_grad[d] = dev_out + (size_t)(d + 1) * pitch;
  hipError_t err = hipSuccess;
  for (int d = 0; d < nd && err == hipSuccess; ++d)
    err = hipMemcpyAsync(static_cast<char*>(block) + off[d], axes[d], s.m[d] * elem, hipMemcpyHostToDevice, l.stream);
  st = INTERPN_HIP_OK;
  for (size_t i0 = 0; i0 < s.m[0] && err == hipSuccess && st == INTERPN_HIP_OK; i0 += rows0) {
    const size_t cnt0 = s.m[0] - i0 < rows0 ? s.m[0] - i0 : rows0;
    const void* sub_axes[8];
    size_t sub_lens[8];
    for (int d = 0; d < nd; ++d) {
      sub_axes[d] = static_cast<char*>(block) + off[d] + (d == 0 ? i0 * elem : 0);
      sub_lens[d] = d == 0 ? cnt0 : s.m[d];
    }
    LatticeShape sub;
    st = lattice_make_shape(sub_axes, sub_lens, (size_t)nd, &sub);
    if (st) break;
    st = lattice_grad_device(h, sub, dev_out, dev_grad, l.stream, 0u, nullptr);
    if (st) break;
    err = hipMemcpyAsync(l.flag_host, h->first_bad, sizeof(unsigned long long), hipMemcpyDeviceToHost, l.stream);
    if (err == hipSuccess) err = hipStreamSynchronize(l.stream);
    if (err != hipSuccess) break;
    const unsigned long long bad = *l.flag_host;
    size_t good = sub.npoints;
    if (bad != kNoBadIndexHost) {
      err = hipMemsetAsync(h->first_bad, 0xFF, sizeof(unsigned long long), l.stream);
      good = (size_t)bad;  // the reference's loop stops here: [0 .. i) written, the rest untouched
      if (first_bad_index) *first_bad_index = (uint64_t)(i0 * per0 + good);
      st = h->desc.unrep_status;
    }
    if (good && err == hipSuccess)
      err = hipMemcpyAsync(static_cast<char*>(out) + i0 * per0 * elem, dev_out, good * elem, hipMemcpyDeviceToHost, l.stream);
    for (int d = 0; d < nd && good && err == hipSuccess; ++d)
      err = hipMemcpyAsync(static_cast<char*>(grad[d]) + i0 * per0 * elem, dev_grad[d], good * elem, hipMemcpyDeviceToHost, l.stream);
    if (err == hipSuccess) err = hipStreamSynchronize(l.stream);
  }
  (void)hipStreamSynchronize(l.stream);  // nothing in flight touches the block when it goes back to the pool
  pool_free(h->device, block);
  if (err != hipSuccess) return hip_fail(err);
  return st;
}

}  // extern "C"
