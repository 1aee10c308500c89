// Gradients of a field set (include/interpn_hip.h, "Gradients of a field set"): the K values and the K x N Jacobian of a
// set at every point.  One launch of k_linear_fields_grad on the set's fused table (linear_fields_grad.h), or K gradient
// evaluations through the K handles into the same blocks.  (C ABI internals, see abi_internal.h.)
#include "abi_internal.h"

using namespace interpn;
using namespace interpn_abi;

namespace {

// Which path a gradient evaluation takes when the caller leaves it to the set (fused = -1): fused wherever the set has the
// table.  Both paths are one-pass kernels (gradients have no sweep form), so the sweep clause of the value rule
// (auto_takes_fused, abi_fields.hip) does not apply.  Its line-fill clause (4 K < 3 ceil(K / P) P -> per field) was measured
// and not adopted (profiles/fields_grad_bench.json, 1e7 points; K handles / fused): the rows where fused loses, 3-D 64^3 f64
// K = 3 (0.94 regular, 0.97 rectilinear), have lines exactly 3/4 full and are outside it; inside it it is right for 3-D f32
// K = 2 (0.89), indifferent for 3-D f32 K = 5 (1.04) and wrong for 2-D 1000^2 f64 K = 2 (1.38).  DESIGN.md, "Field-set
// gradients".
bool grad_auto_takes_fused(const interpn_hip_fields* s) { return s->table != nullptr; }

}  // namespace

namespace interpn_abi {
bool grad_takes_fused(const interpn_hip_fields* s) {
  return s->table && (s->fused == 1 || (s->fused < 0 && grad_auto_takes_fused(s)));
}
}  // namespace interpn_abi

namespace {

// What both entry points check before any device work, in the order of interpn_hip_fields_eval_device / _host.
int fields_grad_checks(const interpn_hip_fields* s, const void* const* obs, const size_t* obs_lens, bool need_lens, size_t nobs,
                       const void* out, size_t out_stride, const void* grad, size_t grad_stride, size_t npoints, bool* nothing) {
  *nothing = false;
  if (!s || s->sub.empty() || (!obs && nobs) || (need_lens && !obs_lens && nobs)) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  const int method = s->sub[0]->desc.method;
  if (method != kLinear && method != kCubic) return INTERPN_HIP_ERR_UNSUPPORTED;  // nearest: no gradient form
  const int st = validate_obs(s->sub[0]->desc, obs_lens, nobs, npoints);
  if (st) return st;
  if (npoints == 0) { *nothing = true; return INTERPN_HIP_OK; }
  if (!out || out_stride < npoints || !grad || grad_stride < npoints) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  for (size_t i = 0; i < nobs; ++i)
    if (!obs[i]) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  return INTERPN_HIP_OK;
}

// The evaluation on validated arguments (the current device is the set's).
int fields_grad_device(interpn_hip_fields* s, const void* const* obs, size_t nobs, void* out, size_t out_stride, void* grad,
                       size_t grad_stride, size_t npoints, hipStream_t hs, unsigned flags, int* path_taken) {
  if (grad_takes_fused(s)) {
    interpn_hip_interp* h0 = s->sub[0];  // its description carries the grid, the axes, the flavour and the options
    HIP_TRY(launch_linear_fields_grad(h0->desc, s->table, (int)s->nfields, obs, out, out_stride, grad, grad_stride, npoints,
                                      h0->first_bad, hs));
    mark_stream(h0, hs);
    s->last_path = INTERPN_HIP_FIELDS_PATH_FUSED;
    if (path_taken) *path_taken = INTERPN_HIP_FIELDS_PATH_FUSED;
    return INTERPN_HIP_OK;
  }
  // the K handles' own tables, as on the value path: once, outside capture, unless the call may not allocate
  if (!s->sub_tables && !(flags & INTERPN_HIP_EVAL_NO_ALLOC) && !stream_capturing(hs)) {
    const int st = ensure_sub_tables(s);
    if (st) return st;
  }
  const size_t elem = s->dtype == kF64 ? 8 : 4;
  const size_t nd = (size_t)s->ndims;
  const bool cubic = s->sub[0]->desc.method == kCubic;
  s->per_field_pending = true;
  s->last_path = INTERPN_HIP_FIELDS_PATH_PER_FIELD;
  for (size_t f = 0; f < s->nfields; ++f) {
    void* rows[8];
    for (size_t d = 0; d < nd; ++d) rows[d] = static_cast<char*>(grad) + (f * nd + d) * grad_stride * elem;
    void* out_f = static_cast<char*>(out) + f * out_stride * elem;
    const int st = cubic ? interpn_hip_eval_cubic_grad_device(s->sub[f], obs, nobs, out_f, rows, npoints, hs)
                         : interpn_hip_eval_grad_device(s->sub[f], obs, nobs, out_f, rows, npoints, hs);
    if (st) return st;
  }
  return INTERPN_HIP_OK;
}

}  // namespace

extern "C" {

int interpn_hip_fields_eval_grad_device(interpn_hip_fields* s, const void* const* obs, size_t nobs, void* out, size_t out_stride,
                                        void* grad, size_t grad_stride, size_t npoints, void* stream, unsigned flags,
                                        int* path_taken) {
  if (path_taken) *path_taken = INTERPN_HIP_FIELDS_PATH_PER_FIELD;
  if (flags & ~(unsigned)INTERPN_HIP_EVAL_NO_ALLOC) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  bool nothing = false;
  const int st = fields_grad_checks(s, obs, nullptr, false, nobs, out, out_stride, grad, grad_stride, npoints, &nothing);
  if (st || nothing) return st;
  DeviceGuard guard(s->device);
  if (!guard.ok()) return INTERPN_HIP_ERR_NO_DEVICE;
  return fields_grad_device(s, obs, nobs, out, out_stride, grad, grad_stride, npoints, static_cast<hipStream_t>(stream), flags,
                            path_taken);
}

int interpn_hip_fields_eval_grad_host(interpn_hip_fields* s, const void* const* obs, const size_t* obs_lens, size_t nobs, void* out,
                                      size_t out_stride, void* grad, size_t grad_stride, size_t nout) {
  bool nothing = false;
  int st = fields_grad_checks(s, obs, obs_lens, true, nobs, out, out_stride, grad, grad_stride, nout, &nothing);
  if (st || nothing) return st;
  DeviceGuard guard(s->device);
  if (!guard.ok()) return INTERPN_HIP_ERR_NO_DEVICE;
  const size_t elem = s->dtype == kF64 ? 8 : 4;
  const size_t nd = (size_t)s->ndims;
  const long long opt_chunk = s->sub[0]->desc.cfg.host_chunk;
  size_t chunk = opt_chunk >= 1 ? (size_t)opt_chunk : ((size_t)2 << 20);
  if (chunk > nout) chunk = nout;
  std::lock_guard<std::mutex> host_lock(s->host_mu);
  if (!s->stream) HIP_TRY(pool_take_kit(s->device, &s->stream, &s->kit_word));
  // the staging of interpn_hip_fields_eval_host (coordinates and value rows), then the K * N gradient rows beside it
  if (s->host_points < chunk) {
    HIP_TRY(hipStreamSynchronize(s->stream));
    pool_free(s->device, s->host_obs);
    pool_free(s->device, s->host_out);
    s->host_obs = s->host_out = nullptr;
    s->host_points = 0;
    HIP_TRY(pool_alloc(s->device, &s->host_obs, nd * chunk * elem));
    HIP_TRY(pool_alloc(s->device, &s->host_out, s->nfields * chunk * elem));
    s->host_points = chunk;
  }
  if (s->host_grad_points < chunk) {
    HIP_TRY(hipStreamSynchronize(s->stream));
    pool_free(s->device, s->host_grad);
    s->host_grad = nullptr;
    s->host_grad_points = 0;
    HIP_TRY(pool_alloc(s->device, &s->host_grad, s->nfields * nd * chunk * elem));
    s->host_grad_points = chunk;
  }
  const size_t cap = s->host_points, gcap = s->host_grad_points;
  char* dev_obs_base = static_cast<char*>(s->host_obs);
  char* dev_out = static_cast<char*>(s->host_out);
  char* dev_grad = static_cast<char*>(s->host_grad);
  const void* dev_obs[8];
  for (size_t begin = 0; begin < nout; begin += chunk) {
    const size_t count = nout - begin < chunk ? nout - begin : chunk;
    // the chunk's coordinates cross PCIe once, whatever the number of fields
    for (size_t d = 0; d < nd; ++d) {
      char* dst = dev_obs_base + d * cap * elem;
      HIP_TRY(hipMemcpyAsync(dst, static_cast<const char*>(obs[d]) + begin * elem, count * elem, hipMemcpyHostToDevice, s->stream));
      dev_obs[d] = dst;
    }
    st = fields_grad_device(s, dev_obs, nobs, dev_out, cap, dev_grad, gcap, count, s->stream, 0u, nullptr);
    if (st) return st;
    uint64_t bad = 0;
    st = interpn_hip_fields_finish(s, s->stream, &bad);
    const bool failed = st == s->sub[0]->desc.unrep_status;
    if (st && !failed) return st;
    // the reference stops at the first failing point: rows written in front of it, untouched behind it
    const size_t good = failed ? (size_t)bad : count;
    if (good)
      for (size_t f = 0; f < s->nfields; ++f) {
        HIP_TRY(hipMemcpyAsync(static_cast<char*>(out) + (f * out_stride + begin) * elem, dev_out + f * cap * elem, good * elem,
                               hipMemcpyDeviceToHost, s->stream));
        for (size_t d = 0; d < nd; ++d)
          HIP_TRY(hipMemcpyAsync(static_cast<char*>(grad) + ((f * nd + d) * grad_stride + begin) * elem,
                                 dev_grad + (f * nd + d) * gcap * elem, good * elem, hipMemcpyDeviceToHost, s->stream));
      }
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (failed) return st;
  }
  return INTERPN_HIP_OK;
}

}  // extern "C"
