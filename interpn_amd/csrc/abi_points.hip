// Point-major observation points (linear_points.h): path choice, the split path's slices and scratch, the device- and
// host-pointer entry points; and the same for their value-and-gradient form (points_grad.h), which shares the slices, the
// scratch rules and the chunk loop.  (C ABI internals, see abi_internal.h.)
#include "abi_internal.h"

using namespace interpn;
using namespace interpn_abi;

namespace {

// Points per chunk of the host form, as interpn_hip_eval_grad_host: upload, evaluate, status word, download.
constexpr size_t kPointsChunk = (size_t)2 << 20;

using Slot = interpn_hip_interp::BinSlot;

// Points per slice of the split path: the coordinates of a slice are bounded like those of the lattice's expanded path.
size_t split_slice(const GridDesc& g, size_t npoints) {
  const size_t elem = g.dtype == kF64 ? 8 : 4;
  size_t slice = kExpandSliceBytes / ((size_t)g.ndims * elem);
  if (slice < kExpandSliceMin) slice = kExpandSliceMin;
  if (g.cfg.points_slice > 0) slice = (size_t)g.cfg.points_slice < 256 ? 256 : (size_t)g.cfg.points_slice;  // testing
  slice &= ~(size_t)255;  // slices begin 16-byte aligned in `out` and in the coordinate arrays (sweep evaluation)
  return npoints < slice ? npoints : slice;
}

// Bytes of the scratch block: one word pair for the first-failing index, then the slice's coordinate arrays.
size_t split_need(const GridDesc& g, size_t npoints) {
  const size_t elem = g.dtype == kF64 ? 8 : 4;
  return 256 + (size_t)g.ndims * align_up(split_slice(g, npoints) * elem, 256);
}

// INTERPN_HIP_POINTS_PATH_* for this call, or -1: option points_path = 1 on a handle without a fused kernel.
int choose_path(const GridDesc& g, size_t stride) {
  const bool fused = points_fused_applies(g);
  if (g.cfg.points_path == 1) return fused ? INTERPN_HIP_POINTS_PATH_FUSED : -1;
  if (g.cfg.points_path == 2) return INTERPN_HIP_POINTS_PATH_SPLIT;
  if (fused) return INTERPN_HIP_POINTS_PATH_FUSED;  // the automatic rule and what it rests on: DESIGN.md section 12
  if (g.ndims == 1 && stride == 1) return INTERPN_HIP_POINTS_PATH_DIRECT;  // already a coordinate array
  return INTERPN_HIP_POINTS_PATH_SPLIT;
}

// What both entry points check, in this order, before any device work; *path: INTERPN_HIP_POINTS_PATH_*.
int points_checks(const interpn_hip_interp* h, const void* pts, size_t stride, size_t npoints, const void* out, bool* nothing,
                  int* path) {
  *nothing = false;
  if (!h) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  if (stride < (size_t)h->desc.ndims) return INTERPN_HIP_ERR_INVALID_ARGUMENT;  // (one_dim handles: ndims = 1)
  if (npoints == 0) { *nothing = true; return INTERPN_HIP_OK; }
  if (!pts || !out) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  if (npoints > (~(size_t)0) / 8 / stride) return INTERPN_HIP_ERR_INVALID_ARGUMENT;  // the block's bytes fit size_t
  *path = choose_path(h->desc, stride);
  return *path < 0 ? INTERPN_HIP_ERR_UNSUPPORTED : INTERPN_HIP_OK;
}

// The split path's frame, shared by the value and the gradient form.  A scratch block of `need` bytes is taken (reserved
// blocks only under capture, allocation unless NO_ALLOC otherwise): one word pair, the slice's ndims coordinate arrays, then
// whatever else the form asked for (`rest`, arrays of `pitch` bytes).  Per slice: k_split_points fills the coordinate
// arrays, `eval(col, rest, pitch, begin, count, &err)` evaluates them (it returns a status and leaves a HIP error in err),
// `after(rest, pitch, begin, count)` follows a slice that went well.  The slice's kernels count failing points from the
// slice's start, so around every slice but the first the word is parked and `begin` added afterwards.
template <typename Eval, typename After>
int split_slices(interpn_hip_interp* h, size_t need, const void* pts, size_t stride, size_t npoints, hipStream_t stream,
                 unsigned flags, Eval eval, After after) {
  const GridDesc& g = h->desc;
  const size_t elem = g.dtype == kF64 ? 8 : 4;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusActive; }
  const bool capturing = cs != hipStreamCaptureStatusNone;
  int why = INTERPN_HIP_WHY_NONE;
  Slot* slot = capturing ? take_slot_captured(h, need, stream)
                         : take_bin_slot(h, need, stream, !(flags & INTERPN_HIP_EVAL_NO_ALLOC), &why);
  if (!slot) return INTERPN_HIP_ERR_OUT_OF_MEMORY;  // no block reserved (interpn_hip_reserve_points[_grad]) and none may be made
  claim_slot(h, slot);
  unsigned char* scratch = static_cast<unsigned char*>(slot->scratch);
  unsigned long long* saved = reinterpret_cast<unsigned long long*>(scratch);
  const size_t slice = split_slice(g, npoints);
  const size_t pitch = align_up(slice * elem, 256);
  void* col[8] = {nullptr};
  for (int d = 0; d < g.ndims; ++d) col[d] = scratch + 256 + (size_t)d * pitch;
  unsigned char* rest = scratch + 256 + (size_t)g.ndims * pitch;
  hipError_t err = hipSuccess;
  int st = INTERPN_HIP_OK;
  for (size_t begin = 0; begin < npoints && err == hipSuccess && st == INTERPN_HIP_OK; begin += slice) {
    const size_t count = npoints - begin < slice ? npoints - begin : slice;
    err = launch_split_points(g, static_cast<const char*>(pts) + begin * stride * elem, stride, col, count, stream);
    if (err == hipSuccess && begin) err = launch_points_bad_begin(h->first_bad, saved, stream);
    if (err != hipSuccess) break;
    st = eval(col, rest, pitch, begin, count, &err);
    if (begin) {  // also behind a failed slice: the parked word goes back
      const hipError_t e2 = launch_points_bad_end(h->first_bad, saved, (unsigned long long)begin, stream);
      if (err == hipSuccess) err = e2;
    }
    if (err == hipSuccess && st == INTERPN_HIP_OK) err = after(rest, pitch, begin, count);
  }
  if (capturing) release_slot_captured(h, slot);
  else release_bin_slot(h, slot, stream, false);
  if (err != hipSuccess || st != INTERPN_HIP_OK) {
    (void)hipGetLastError();
    std::lock_guard<std::mutex> lk(h->marks_mu);
    h->sync_device_at_destroy = true;  // part of the sequence may be in flight without a mark behind it
    return err != hipSuccess ? hip_fail(err) : st;
  }
  mark_stream(h, stream);
  return INTERPN_HIP_OK;
}

int split_device(interpn_hip_interp* h, const void* pts, size_t stride, size_t npoints, void* out, hipStream_t stream, unsigned flags) {
  const size_t elem = h->desc.dtype == kF64 ? 8 : 4;
  return split_slices(
      h, split_need(h->desc, npoints), pts, stride, npoints, stream, flags,
      [&](void* const* col, unsigned char*, size_t, size_t begin, size_t count, hipError_t*) {
        return interpn_hip_eval_device_ex(h, col, (size_t)h->desc.ndims, static_cast<char*>(out) + begin * elem, count, stream,
                                          flags & INTERPN_HIP_EVAL_NO_ALLOC, nullptr, nullptr);
      },
      [](unsigned char*, size_t, size_t, size_t) { return hipSuccess; });
}

// One block of points on device memory.  Arguments are validated; the current device is the handle's.
int points_device(interpn_hip_interp* h, int path, const void* pts, size_t stride, size_t npoints, void* out, hipStream_t stream,
                  unsigned flags) {
  int st = INTERPN_HIP_OK;
  if (path == INTERPN_HIP_POINTS_PATH_FUSED) {
    HIP_TRY(launch_linear_points(h->desc, pts, stride, out, npoints, h->first_bad, stream));
    h->desc.last_binned = 0;
    h->evals_in_place.fetch_add(1);
    mark_stream(h, stream);
  } else if (path == INTERPN_HIP_POINTS_PATH_DIRECT) {
    st = interpn_hip_eval_device_ex(h, &pts, 1, out, npoints, stream, flags, nullptr, nullptr);
  } else {
    st = split_device(h, pts, stride, npoints, out, stream, flags);
  }
  if (st == INTERPN_HIP_OK) h->desc.last_points_path = path;
  return st;
}


// ---- value and gradient (points_grad.h) --------------------------------------------------------------------------------

// Bytes of the gradient form's scratch block: the word pair, the slice's coordinate arrays, then its component arrays.
size_t split_grad_need(const GridDesc& g, size_t npoints) {
  const size_t elem = g.dtype == kF64 ? 8 : 4;
  return 256 + 2 * (size_t)g.ndims * align_up(split_slice(g, npoints) * elem, 256);
}

int choose_grad_path(const GridDesc& g, size_t stride, size_t gstride) {
  const bool fused = points_grad_fused_applies(g, stride, gstride);
  if (g.cfg.points_path == 1) return fused ? INTERPN_HIP_POINTS_PATH_FUSED : -1;
  if (g.cfg.points_path == 2) return INTERPN_HIP_POINTS_PATH_SPLIT;
  if (fused) return INTERPN_HIP_POINTS_PATH_FUSED;  // the automatic rule and what it rests on: DESIGN.md section 14
  if (g.ndims == 1 && stride == 1 && gstride == 1) return INTERPN_HIP_POINTS_PATH_DIRECT;  // a coordinate and a component array
  return INTERPN_HIP_POINTS_PATH_SPLIT;
}

// What both gradient entry points check, in this order, before any device work; *path: INTERPN_HIP_POINTS_PATH_*.
int points_grad_checks(const interpn_hip_interp* h, const void* pts, size_t stride, size_t npoints, const void* out, const void* grad,
                       size_t gstride, bool* nothing, int* path) {
  *nothing = false;
  if (!h) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  if (h->desc.method != kLinear && h->desc.method != kCubic) return INTERPN_HIP_ERR_UNSUPPORTED;  // nearest, one_dim: no gradient form
  if (stride < (size_t)h->desc.ndims || gstride < (size_t)h->desc.ndims) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  if (npoints == 0) { *nothing = true; return INTERPN_HIP_OK; }
  if (!pts || !out || !grad) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  if (npoints > (~(size_t)0) / 8 / stride || npoints > (~(size_t)0) / 8 / gstride) return INTERPN_HIP_ERR_INVALID_ARGUMENT;  // both blocks' bytes fit size_t
  *path = choose_grad_path(h->desc, stride, gstride);
  return *path < 0 ? INTERPN_HIP_ERR_UNSUPPORTED : INTERPN_HIP_OK;
}

// The split path of the gradient form: the column form's launch (abi_grad.hip) writes the value straight to `out + begin`
// and the components to the ndims arrays behind the coordinate arrays; k_join_grad interleaves those into the rows.
int split_grad_device(interpn_hip_interp* h, const void* pts, size_t stride, size_t npoints, void* out, void* grad, size_t gstride,
                      hipStream_t stream, unsigned flags) {
  const GridDesc& g = h->desc;
  const size_t elem = g.dtype == kF64 ? 8 : 4;
  void* comp[8] = {nullptr};
  return split_slices(
      h, split_grad_need(g, npoints), pts, stride, npoints, stream, flags,
      [&](void* const* col, unsigned char* rest, size_t pitch, size_t begin, size_t count, hipError_t* err) {
        for (int d = 0; d < g.ndims; ++d) comp[d] = rest + (size_t)d * pitch;
        *err = launch_grad(g, col, static_cast<char*>(out) + begin * elem, comp, count, h->first_bad, stream);
        return (int)INTERPN_HIP_OK;
      },
      [&](unsigned char*, size_t, size_t begin, size_t count) {
        return launch_join_grad(g, comp, static_cast<char*>(grad) + begin * gstride * elem, gstride, count, stream);
      });
}

// One block of points on device memory, value and gradient.  Arguments are validated; the current device is the handle's.
int points_grad_device(interpn_hip_interp* h, int path, const void* pts, size_t stride, size_t npoints, void* out, void* grad,
                       size_t gstride, hipStream_t stream, unsigned flags) {
  if (path == INTERPN_HIP_POINTS_PATH_SPLIT) {
    const int st = split_grad_device(h, pts, stride, npoints, out, grad, gstride, stream, flags);  // marks the stream itself
    if (st) return st;
  } else {
    if (path == INTERPN_HIP_POINTS_PATH_FUSED)
      HIP_TRY(launch_points_grad(h->desc, pts, stride, out, grad, gstride, npoints, h->first_bad, stream));
    else
      HIP_TRY(launch_grad(h->desc, &pts, out, &grad, npoints, h->first_bad, stream));
    mark_stream(h, stream);
  }
  h->desc.last_binned = 0;
  h->evals_in_place.fetch_add(1);
  h->desc.last_points_path = path;
  return INTERPN_HIP_OK;
}

// The host forms' chunk loop, shared by the value and the gradient form, on the handle's first host lane.  One pool block
// holds a chunk's rows and, behind them, `result_bytes(chunk)` bytes of results.  Per chunk: one copy of the interleaved
// rows up, `eval(rows, results, chunk, count, stream)`, the status word, then `download(results, chunk, begin, good, stream)`
// for the `good` points in front of the first failing one.  The reference's loop stops at the first failing point:
// results [0..i) are written, the rest is left as it was.
template <typename Bytes, typename Eval, typename Download>
int host_chunks(interpn_hip_interp* h, const void* pts, size_t point_stride, size_t npoints, Bytes result_bytes, Eval eval,
                Download download) {
  std::lock_guard<std::mutex> host_lock(h->host_mu);
  DeviceGuard guard(h->device);
  if (!guard.ok()) return INTERPN_HIP_ERR_NO_DEVICE;
  interpn_hip_interp::HostLane& l = h->lane[0];
  if (!l.stream) HIP_TRY(pool_take_kit(h->device, &l.stream, &l.flag_host));
  const size_t elem = h->desc.dtype == kF64 ? 8 : 4;
  const size_t nd = (size_t)h->desc.ndims;
  size_t chunk = npoints < kPointsChunk ? npoints : kPointsChunk;
  if (h->desc.cfg.host_chunk >= 1)  // testing: force small chunks
    chunk = (size_t)h->desc.cfg.host_chunk < npoints ? (size_t)h->desc.cfg.host_chunk : npoints;
  // a wide record would make the rows of a chunk large: keep the upload of a chunk within 256 MiB
  const size_t cap = ((size_t)256 << 20) / (point_stride * elem);
  if (chunk > cap) chunk = cap ? cap : 1;
  const size_t rows_bytes = align_up(chunk * point_stride * elem, 256);
  void* block = nullptr;
  if (pool_alloc(h->device, &block, rows_bytes + result_bytes(chunk)) != hipSuccess) { (void)hipGetLastError(); return INTERPN_HIP_ERR_OUT_OF_MEMORY; }
  char* results = static_cast<char*>(block) + rows_bytes;
  hipError_t err = hipSuccess;
  int st = INTERPN_HIP_OK;
  for (size_t begin = 0; begin < npoints && err == hipSuccess && st == INTERPN_HIP_OK; begin += chunk) {
    const size_t count = npoints - begin < chunk ? npoints - begin : chunk;
    // one copy of the interleaved rows; the last row ends with its last coordinate
    err = hipMemcpyAsync(block, static_cast<const char*>(pts) + begin * point_stride * elem, ((count - 1) * point_stride + nd) * elem,
                         hipMemcpyHostToDevice, l.stream);
    if (err != hipSuccess) break;
    st = eval(block, results, chunk, count, l.stream);
    if (st) break;
    err = hipMemcpyAsync(l.flag_host, h->first_bad, sizeof(unsigned long long), hipMemcpyDeviceToHost, l.stream);
    if (err == hipSuccess) err = hipStreamSynchronize(l.stream);
    if (err != hipSuccess) break;
    const unsigned long long bad = *l.flag_host;
    size_t good = count;
    if (bad != kNoBadIndexHost) {
      err = hipMemsetAsync(h->first_bad, 0xFF, sizeof(unsigned long long), l.stream);
      good = (size_t)bad;
      st = h->desc.unrep_status;
    }
    if (good && err == hipSuccess) err = download(results, chunk, begin, good, l.stream);
    if (err == hipSuccess) err = hipStreamSynchronize(l.stream);
  }
  (void)hipStreamSynchronize(l.stream);  // nothing in flight touches the block when it goes back to the pool
  pool_free(h->device, block);
  if (err != hipSuccess) return hip_fail(err);
  return st;
}

}  // namespace

extern "C" {

int interpn_hip_eval_points_device(interpn_hip_interp* h, const void* pts, size_t point_stride, size_t npoints, void* out,
                                   void* stream, unsigned flags, int* path_taken) {
  if (path_taken) *path_taken = INTERPN_HIP_POINTS_PATH_SPLIT;
  if (flags & ~(unsigned)INTERPN_HIP_EVAL_NO_ALLOC) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  bool nothing = false;
  int path = INTERPN_HIP_POINTS_PATH_SPLIT;
  const int st0 = points_checks(h, pts, point_stride, npoints, out, &nothing, &path);
  if (st0 || nothing) return st0;
  DeviceGuard guard(h->device);
  if (!guard.ok()) return INTERPN_HIP_ERR_NO_DEVICE;
  const int st = points_device(h, path, pts, point_stride, npoints, out, static_cast<hipStream_t>(stream), flags);
  if (st == INTERPN_HIP_OK && path_taken) *path_taken = path;
  return st;
}

int interpn_hip_reserve_points(interpn_hip_interp* h, size_t npoints, int nstreams) {
  if (!h || nstreams < 0) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  if ((size_t)nstreams > interpn_hip_interp::kMaxBinSlots) nstreams = (int)interpn_hip_interp::kMaxBinSlots;
  if (npoints == 0 || nstreams == 0) return INTERPN_HIP_OK;
  DeviceGuard guard(h->device);
  if (!guard.ok()) return INTERPN_HIP_ERR_NO_DEVICE;
  return reserve_slots(h, split_need(h->desc, npoints), nstreams);
}

int interpn_hip_eval_points_host(interpn_hip_interp* h, const void* pts, size_t point_stride, size_t npoints, void* out) {
  bool nothing = false;
  int path = INTERPN_HIP_POINTS_PATH_SPLIT;
  const int st0 = points_checks(h, pts, point_stride, npoints, out, &nothing, &path);
  if (st0 || nothing) return st0;
  const size_t elem = h->desc.dtype == kF64 ? 8 : 4;
  return host_chunks(
      h, pts, point_stride, npoints, [&](size_t chunk) { return chunk * elem; },
      [&](void* rows, char* dev_out, size_t, size_t count, hipStream_t s) {
        return points_device(h, path, rows, point_stride, count, dev_out, s, 0u);
      },
      [&](char* dev_out, size_t, size_t begin, size_t good, hipStream_t s) {
        return hipMemcpyAsync(static_cast<char*>(out) + begin * elem, dev_out, good * elem, hipMemcpyDeviceToHost, s);
      });
}

int interpn_hip_eval_points_grad_device(interpn_hip_interp* h, const void* pts, size_t point_stride, size_t npoints, void* out,
                                        void* grad, size_t grad_stride, void* stream, unsigned flags, int* path_taken) {
  if (path_taken) *path_taken = INTERPN_HIP_POINTS_PATH_SPLIT;
  if (flags & ~(unsigned)INTERPN_HIP_EVAL_NO_ALLOC) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  bool nothing = false;
  int path = INTERPN_HIP_POINTS_PATH_SPLIT;
  const int st0 = points_grad_checks(h, pts, point_stride, npoints, out, grad, grad_stride, &nothing, &path);
  if (st0 || nothing) return st0;
  DeviceGuard guard(h->device);
  if (!guard.ok()) return INTERPN_HIP_ERR_NO_DEVICE;
  const int st = points_grad_device(h, path, pts, point_stride, npoints, out, grad, grad_stride, static_cast<hipStream_t>(stream), flags);
  if (st == INTERPN_HIP_OK && path_taken) *path_taken = path;
  return st;
}

int interpn_hip_reserve_points_grad(interpn_hip_interp* h, size_t npoints, int nstreams) {
  if (!h || nstreams < 0) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  if ((size_t)nstreams > interpn_hip_interp::kMaxBinSlots) nstreams = (int)interpn_hip_interp::kMaxBinSlots;
  if (npoints == 0 || nstreams == 0) return INTERPN_HIP_OK;
  DeviceGuard guard(h->device);
  if (!guard.ok()) return INTERPN_HIP_ERR_NO_DEVICE;
  return reserve_slots(h, split_grad_need(h->desc, npoints), nstreams);
}

int interpn_hip_eval_points_grad_host(interpn_hip_interp* h, const void* pts, size_t point_stride, size_t npoints, void* out,
                                      void* grad, size_t grad_stride) {
  bool nothing = false;
  int path = INTERPN_HIP_POINTS_PATH_SPLIT;
  const int st0 = points_grad_checks(h, pts, point_stride, npoints, out, grad, grad_stride, &nothing, &path);
  if (st0 || nothing) return st0;
  const size_t elem = h->desc.dtype == kF64 ? 8 : 4;
  const size_t nd = (size_t)h->desc.ndims;
  // The chunk's gradient rows are packed on the device whatever the caller's stride; the column form of one point per row is
  // the packed form, so the direct path (N = 1) takes it as it is.
  const int dev_path = choose_grad_path(h->desc, point_stride, nd);
  if (dev_path < 0) return INTERPN_HIP_ERR_UNSUPPORTED;
  // results of a chunk: its values, then its gradient rows
  auto out_bytes = [&](size_t chunk) { return align_up(chunk * elem, 256); };
  return host_chunks(
      h, pts, point_stride, npoints, [&](size_t chunk) { return out_bytes(chunk) + chunk * nd * elem; },
      [&](void* rows, char* dev_out, size_t chunk, size_t count, hipStream_t s) {
        return points_grad_device(h, dev_path, rows, point_stride, count, dev_out, dev_out + out_bytes(chunk), nd, s, 0u);
      },
      [&](char* dev_out, size_t chunk, size_t begin, size_t good, hipStream_t s) {
        hipError_t err = hipMemcpyAsync(static_cast<char*>(out) + begin * elem, dev_out, good * elem, hipMemcpyDeviceToHost, s);
        if (err != hipSuccess) return err;
        char* dst = static_cast<char*>(grad) + begin * grad_stride * elem;
        const char* dev_grad = dev_out + out_bytes(chunk);
        if (grad_stride == nd) return hipMemcpyAsync(dst, dev_grad, good * nd * elem, hipMemcpyDeviceToHost, s);
        // the caller's rows are wider: columns d >= ndims are never written
        return hipMemcpy2DAsync(dst, grad_stride * elem, dev_grad, nd * elem, nd * elem, good, hipMemcpyDeviceToHost, s);
      });
}

}  // extern "C"
