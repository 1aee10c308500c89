// Value and gradient of a multilinear handle (interpn_hip_eval_grad_device / _host) and of a multicubic handle
// (interpn_hip_eval_cubic_grad_device / _host): one set of checks and one host chunk loop, the method picks the launcher.
// (C ABI internals, see abi_internal.h.)
#include "abi_internal.h"

using namespace interpn;
using namespace interpn_abi;

namespace {

// Points per chunk of the host form: upload, one kernel, status word, download, chunk after chunk on the handle's first
// host lane.  (Simpler than eval_host's two-lane pipeline: a gradient call downloads N + 1 arrays per chunk, the
// transfers dominate either way.)
constexpr size_t kGradChunkPoints = (size_t)2 << 20;

struct PoolBlock {
  int device;
  void* p = nullptr;
  explicit PoolBlock(int dev) : device(dev) {}
  ~PoolBlock() { if (p) pool_free(device, p); }
};

// The checks of interpn_hip_eval_device / _host, with the gradient arrays; 0 = go on
int grad_checks(interpn_hip_interp* h, int method, const void* const* obs, const size_t* obs_lens, bool need_lens, size_t nobs,
                void* out, void* const* grad, size_t npoints, bool* nothing) {
  *nothing = false;
  if (!h || (!obs && nobs) || (need_lens && !obs_lens && nobs)) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  if (h->desc.method != method) return INTERPN_HIP_ERR_UNSUPPORTED;  // each entry point serves one method; nearest, one_dim: no gradient form
  const int st = validate_obs(h->desc, obs_lens, nobs, npoints);
  if (st) return st;
  if (npoints == 0) { *nothing = true; return INTERPN_HIP_OK; }
  if (!out || !grad) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  for (size_t i = 0; i < nobs; ++i)
    if (!obs[i] || !grad[i]) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  return INTERPN_HIP_OK;
}

}  // namespace

namespace interpn_abi {

hipError_t launch_grad(const GridDesc& g, const void* const* obs, void* out, void* const* grad, size_t npts,
                       unsigned long long* first_bad, hipStream_t stream) {
  return g.method == kCubic ? launch_cubic_grad(g, obs, out, grad, npts, first_bad, stream)
                            : launch_linear_grad(g, obs, out, grad, npts, first_bad, stream);
}

}  // namespace interpn_abi

namespace {

int grad_device(interpn_hip_interp* h, int method, const void* const* obs, size_t nobs, void* out, void* const* grad,
                size_t npoints, void* stream) {
  bool nothing = false;
  const int st = grad_checks(h, method, obs, nullptr, false, nobs, out, grad, npoints, &nothing);
  if (st || nothing) return st;
  DeviceGuard guard(h->device);
  if (!guard.ok()) return INTERPN_HIP_ERR_NO_DEVICE;
  HIP_TRY(launch_grad(h->desc, obs, out, grad, npoints, h->first_bad, static_cast<hipStream_t>(stream)));
  h->desc.last_binned = 0;
  h->evals_in_place.fetch_add(1);
  mark_stream(h, static_cast<hipStream_t>(stream));
  return INTERPN_HIP_OK;
}

int grad_host(interpn_hip_interp* h, int method, const void* const* obs, const size_t* obs_lens, size_t nobs, void* out, size_t nout,
              void* const* grad) {
  bool nothing = false;
  const int st0 = grad_checks(h, method, obs, obs_lens, true, nobs, out, grad, nout, &nothing);
  if (st0 || nothing) return st0;
  std::lock_guard<std::mutex> host_lock(h->host_mu);
  DeviceGuard guard(h->device);
  if (!guard.ok()) return INTERPN_HIP_ERR_NO_DEVICE;
  const size_t elem = h->desc.dtype == kF64 ? 8 : 4;
  const int nd = h->desc.ndims;
  size_t chunk = nout < kGradChunkPoints ? nout : kGradChunkPoints;
  if (h->desc.cfg.host_chunk >= 1)  // testing: force small chunks
    chunk = (size_t)h->desc.cfg.host_chunk < nout ? (size_t)h->desc.cfg.host_chunk : nout;
  const int st = ensure_lane(h, 0, chunk);
  if (st) return st;
  const interpn_hip_interp::HostLane& l = h->lane[0];
  PoolBlock gbuf(h->device);
  if (pool_alloc(h->device, &gbuf.p, (size_t)nd * chunk * elem) != hipSuccess) {
    (void)hipGetLastError();
    gbuf.p = nullptr;
    return INTERPN_HIP_ERR_OUT_OF_MEMORY;
  }
  const void* dev_obs[8];
  void* dev_grad[8];
  for (int d = 0; d < nd; ++d) {
    dev_obs[d] = (char*)l.obs + (size_t)d * l.points * elem;
    dev_grad[d] = (char*)gbuf.p + (size_t)d * chunk * elem;
  }
  // The reference's loop stops at the first failing point: out[0..i) and grad[d][0..i) written, the rest untouched.
  for (size_t begin = 0; begin < nout; begin += chunk) {
    const size_t count = (nout - begin) < chunk ? (nout - begin) : chunk;
    for (int d = 0; d < nd; ++d)
      HIP_TRY(hipMemcpyAsync(const_cast<void*>(dev_obs[d]), (const char*)obs[d] + begin * elem, count * elem, hipMemcpyHostToDevice, l.stream));
    HIP_TRY(launch_grad(h->desc, dev_obs, l.out, dev_grad, count, l.flag_dev, l.stream));
    HIP_TRY(hipMemcpyAsync(l.flag_host, l.flag_dev, sizeof(unsigned long long), hipMemcpyDeviceToHost, l.stream));
    HIP_TRY(hipStreamSynchronize(l.stream));
    const unsigned long long bad = *l.flag_host;
    size_t good = count;
    if (bad != kNoBadIndexHost) {
      HIP_TRY(hipMemsetAsync(l.flag_dev, 0xFF, sizeof(unsigned long long), l.stream));
      good = (size_t)bad;
    }
    if (good) {
      HIP_TRY(hipMemcpyAsync((char*)out + begin * elem, l.out, good * elem, hipMemcpyDeviceToHost, l.stream));
      for (int d = 0; d < nd; ++d)
        HIP_TRY(hipMemcpyAsync((char*)grad[d] + begin * elem, dev_grad[d], good * elem, hipMemcpyDeviceToHost, l.stream));
    }
    HIP_TRY(hipStreamSynchronize(l.stream));
    if (bad != kNoBadIndexHost) return h->desc.unrep_status;
  }
  return INTERPN_HIP_OK;
}

}  // namespace

extern "C" {

int interpn_hip_eval_grad_device(interpn_hip_interp* h, const void* const* obs, size_t nobs, void* out, void* const* grad,
                                 size_t npoints, void* stream) {
  return grad_device(h, kLinear, obs, nobs, out, grad, npoints, stream);
}

int interpn_hip_eval_grad_host(interpn_hip_interp* h, const void* const* obs, const size_t* obs_lens, size_t nobs, void* out,
                               size_t nout, void* const* grad) {
  return grad_host(h, kLinear, obs, obs_lens, nobs, out, nout, grad);
}

int interpn_hip_eval_cubic_grad_device(interpn_hip_interp* h, const void* const* obs, size_t nobs, void* out, void* const* grad,
                                       size_t npoints, void* stream) {
  return grad_device(h, kCubic, obs, nobs, out, grad, npoints, stream);
}

int interpn_hip_eval_cubic_grad_host(interpn_hip_interp* h, const void* const* obs, const size_t* obs_lens, size_t nobs, void* out,
                                     size_t nout, void* const* grad) {
  return grad_host(h, kCubic, obs, obs_lens, nobs, out, nout, grad);
}

}  // extern "C"
