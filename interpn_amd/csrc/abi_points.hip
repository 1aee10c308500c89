// Point-major observation points (linear_points.h): path choice, the split path's slices and scratch, the device- and
// host-pointer entry points.  (C ABI internals, see abi_internal.h.)
#include "abi_internal.h"

using namespace interpn;
using namespace interpn_abi;

namespace {

// Points per chunk of the host form, as interpn_hip_eval_grad_host: upload, evaluate, status word, download.
constexpr size_t kPointsChunk = (size_t)2 << 20;

using Slot = interpn_hip_interp::BinSlot;

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

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

int split_device(interpn_hip_interp* h, const void* pts, size_t stride, size_t npoints, void* out, hipStream_t stream, unsigned flags) {
  const GridDesc& g = h->desc;
  const size_t elem = g.dtype == kF64 ? 8 : 4;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusActive; }
  const bool capturing = cs != hipStreamCaptureStatusNone;
  int why = INTERPN_HIP_WHY_NONE;
  Slot* slot = capturing ? take_slot_captured(h, split_need(g, npoints), stream)
                         : take_bin_slot(h, split_need(g, npoints), stream, !(flags & INTERPN_HIP_EVAL_NO_ALLOC), &why);
  if (!slot) return INTERPN_HIP_ERR_OUT_OF_MEMORY;  // no block reserved (interpn_hip_reserve_points) and none may be made
  claim_slot(h, slot);
  unsigned char* scratch = static_cast<unsigned char*>(slot->scratch);
  unsigned long long* saved = reinterpret_cast<unsigned long long*>(scratch);
  const size_t slice = split_slice(g, npoints);
  const size_t pitch = align_up(slice * elem, 256);
  void* dst[8] = {nullptr};
  for (int d = 0; d < g.ndims; ++d) dst[d] = scratch + 256 + (size_t)d * pitch;
  hipError_t err = hipSuccess;
  int st = INTERPN_HIP_OK;
  for (size_t begin = 0; begin < npoints && err == hipSuccess && st == INTERPN_HIP_OK; begin += slice) {
    const size_t count = npoints - begin < slice ? npoints - begin : slice;
    err = launch_split_points(g, static_cast<const char*>(pts) + begin * stride * elem, stride, dst, count, stream);
    // the slice's kernels count failing points from the slice's start: park what the word holds, add `begin` afterwards
    if (err == hipSuccess && begin) err = launch_points_bad_begin(h->first_bad, saved, stream);
    if (err != hipSuccess) break;
    st = interpn_hip_eval_device_ex(h, dst, (size_t)g.ndims, static_cast<char*>(out) + begin * elem,
                                    count, stream, flags & INTERPN_HIP_EVAL_NO_ALLOC, nullptr, nullptr);
    if (begin) {  // also behind a failed slice: the parked word goes back
      const hipError_t e2 = launch_points_bad_end(h->first_bad, saved, (unsigned long long)begin, stream);
      if (err == hipSuccess) err = e2;
    }
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
  // one block: the chunk's rows, then its results
  const size_t rows_bytes = align_up(chunk * point_stride * elem, 256);
  void* block = nullptr;
  if (pool_alloc(h->device, &block, rows_bytes + chunk * elem) != hipSuccess) { (void)hipGetLastError(); return INTERPN_HIP_ERR_OUT_OF_MEMORY; }
  char* dev_out = static_cast<char*>(block) + rows_bytes;
  hipError_t err = hipSuccess;
  int st = INTERPN_HIP_OK;
  // The reference's loop stops at the first failing point: out[0..i) written, the rest untouched.
  for (size_t begin = 0; begin < npoints && err == hipSuccess && st == INTERPN_HIP_OK; begin += chunk) {
    const size_t count = npoints - begin < chunk ? npoints - begin : chunk;
    // one copy of the interleaved rows; the last row ends with its last coordinate
    err = hipMemcpyAsync(block, static_cast<const char*>(pts) + begin * point_stride * elem, ((count - 1) * point_stride + nd) * elem,
                         hipMemcpyHostToDevice, l.stream);
    if (err != hipSuccess) break;
    st = points_device(h, path, block, point_stride, count, dev_out, l.stream, 0u);
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
    if (good && err == hipSuccess)
      err = hipMemcpyAsync(static_cast<char*>(out) + begin * elem, dev_out, good * elem, hipMemcpyDeviceToHost, l.stream);
    if (err == hipSuccess) err = hipStreamSynchronize(l.stream);
  }
  (void)hipStreamSynchronize(l.stream);  // nothing in flight touches the block when it goes back to the pool
  pool_free(h->device, block);
  if (err != hipSuccess) return hip_fail(err);
  return st;
}

}  // extern "C"
