// Kernel dispatch of one evaluation and stream marks (what interpn_hip_destroy waits for).
// (C ABI internals, see abi_internal.h.)
#include "abi_internal.h"

using namespace interpn;
using namespace interpn_abi;

namespace interpn_abi {

template <typename T>
hipError_t launch(const GridDesc& g, const T* const* obs, T* out, size_t npts, unsigned long long* first_bad,
                  hipStream_t stream) {
  if (npts == 0) return hipSuccess;
  if (g.method == kNearest) return launch_nearest<T>(g, obs, out, npts, first_bad, stream);
  if (g.cfg.force_generic || !fast_path(g)) return launch_generic<T>(g, obs, out, npts, first_bad, stream);
  if (g.method == kLinear)
    return g.kind == kRegular ? launch_linear_regular<T>(g, obs, out, npts, first_bad, stream)
                              : launch_linear_rectilinear<T>(g, obs, out, npts, first_bad, stream);
  return g.kind == kRegular ? launch_cubic_regular<T>(g, obs, out, npts, first_bad, stream)
                            : launch_cubic_rectilinear<T>(g, obs, out, npts, first_bad, stream);
}

hipError_t launch_any(const GridDesc& g, const void* const* obs, void* out, size_t npts,
                      unsigned long long* first_bad, hipStream_t stream) {
  if (is_one_dim(g.method)) return launch_one_dim(g, obs[0], out, npts, first_bad, stream);
  if (g.bricks && npts && g.method == kCubic && !g.cfg.force_generic) {
    if (g.dtype == kF64)
      return launch_cubic_brick<double>(g, reinterpret_cast<const double* const*>(obs), static_cast<double*>(out),
                                        npts, first_bad, stream);
    return launch_cubic_brick<float>(g, reinterpret_cast<const float* const*>(obs), static_cast<float*>(out), npts,
                                     first_bad, stream);
  }
  if (g.bricks && npts && g.ndims == 1 && g.method == kLinear && g.rec1_buckets && !g.cfg.force_generic) {
    if (g.dtype == kF64)
      return launch_linear1_records<double>(g, reinterpret_cast<const double* const*>(obs), static_cast<double*>(out), npts, stream);
    return launch_linear1_records<float>(g, reinterpret_cast<const float* const*>(obs), static_cast<float*>(out), npts, stream);
  }
  if (g.bricks && npts && g.ndims == 2 && !g.cfg.force_generic) {
    if (g.dtype == kF64)
      return launch_linear2_brick<double>(g, reinterpret_cast<const double* const*>(obs), static_cast<double*>(out),
                                          npts, first_bad, stream);
    return launch_linear2_brick<float>(g, reinterpret_cast<const float* const*>(obs), static_cast<float*>(out), npts,
                                       first_bad, stream);
  }
  if (g.bricks && npts && !g.cfg.force_generic) {
    if (g.dtype == kF64)
      return launch_linear_brick<double>(g, reinterpret_cast<const double* const*>(obs), static_cast<double*>(out),
                                         npts, first_bad, stream);
    return launch_linear_brick<float>(g, reinterpret_cast<const float* const*>(obs), static_cast<float*>(out), npts,
                                      first_bad, stream);
  }
  if (g.dtype == kF64)
    return launch<double>(g, reinterpret_cast<const double* const*>(obs), static_cast<double*>(out), npts, first_bad, stream);
  return launch<float>(g, reinterpret_cast<const float* const*>(obs), static_cast<float*>(out), npts, first_bad, stream);
}

// Remember that device-pointer work was enqueued on `stream` (see interpn_hip_interp::marks).
// No allocation, copy, synchronisation or stream command: the stream is noted, and
// interpn_hip_destroy waits for it.  A stream under capture is never touched, so eval_device stays
// graph-capturable.
void mark_stream(interpn_hip_interp* h, hipStream_t stream) { scratch_slots::mark_stream(*h, stream); }

}  // namespace interpn_abi
