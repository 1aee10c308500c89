// Internals shared by the translation units of the C ABI (include/interpn_hip.h): the handle, the
// per-device pool, validation in the reference's order, and the entry points the units call in each
// other.  Host logic only.  Split (round 4) from one 2 200-line file into
//   abi_pool.hip      per-device pool of blocks, streams, pinned words; device properties
//   abi_layout.hip    which re-laid copy of the grid a handle keeps (bricks, tiles, 1-D records)
//   abi_options.hip   per-handle options, kernel name, table size
//   abi_create.hip    create / replicate / destroy, status strings
//   abi_launch.hip    kernel dispatch of one evaluation, stream marks
//   abi_binned.hip    sorted (binned / column) evaluation of device-resident batches
//   abi_host.hip      host-pointer pipeline, small-batch path, finish, one-shot entry points
//   abi_bounds.hip    check_bounds
//   abi_sharded.hip   single-process multi-GPU forms
//   abi_grad.hip      value and gradient of a multilinear or multicubic handle (eval_grad_* / eval_cubic_grad_*)
//   abi_fields.hip    field sets: creation, column and point-major forms, options
//   abi_fields_grad.hip  values and Jacobian of a field set (fields_eval_grad_device / _host)
//   abi_fields_points_grad.hip  point-major values and Jacobian of a field set (fields_eval_points_grad_device / _host,
//                     fields_reserve_points_grad)
//   abi_fields_lattice.hip  field sets on a lattice (fields_eval_lattice_device / _host, fields_reserve_lattice, fields_lattice_plan)
//   abi_lattice_grad.hip  value and gradient on a lattice (eval_lattice_grad_device / _host, lattice_grad_plan)
//   abi_fields_lattice_grad.hip  values and Jacobian of a field set on a lattice (fields_eval_lattice_grad_device / _host,
//                     fields_reserve_lattice_grad, fields_lattice_grad_plan)
//   scratch_slots.h   (no HIP in it) scratch blocks between streams and stream marks: settle / take / release / reserve /
//                     mark / the wait at destroy, against a runtime type; HipRuntime below is the product's
//   abi_points.hip    point-major observation points (eval_points_device / _host, reserve_points) and their gradient form
//                     (eval_points_grad_device / _host, reserve_points_grad)
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <condition_variable>
#include <cctype>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/interpn_hip.h"
#include "interpn_host.h"
#include "scratch_slots.h"

namespace interpn {
// Multilinear value and gradient in one pass (k_linear_grad.hip, linear_grad.h): `grad` is a host array of ndims device
// pointers.  The fused kernel for N = 2, 3 on the handle's re-laid table, the runtime-N kernel on `vals` otherwise.
hipError_t launch_linear_grad(const GridDesc& g, const void* const* obs, void* out, void* const* grad, size_t npts,
                              unsigned long long* first_bad, hipStream_t stream);
// Multicubic value and gradient in one pass (k_cubic_grad.hip, cubic_grad.h), same arguments: the fused kernel for N = 2, 3
// on the handle's tiled table, the runtime-N kernel on `vals` otherwise.
hipError_t launch_cubic_grad(const GridDesc& g, const void* const* obs, void* out, void* const* grad, size_t npts,
                             unsigned long long* first_bad, hipStream_t stream);
// Point-major observation points (k_linear_points.hip, linear_points.h): coordinate d of point i at pts[i * stride + d].
// The fused kernel (N = 2, 3 multilinear on the handle's re-laid table); the de-interleaving of a slice into ndims
// coordinate arrays (`dst`: host array of device pointers); and the two one-lane kernels around a slice that starts at
// point `begin` of its call, which keep the first-failing-index word counting from the call's first point.
bool points_fused_applies(const GridDesc& g);
hipError_t launch_linear_points(const GridDesc& g, const void* pts, size_t stride, void* out, size_t npts,
                                unsigned long long* first_bad, hipStream_t stream);
hipError_t launch_split_points(const GridDesc& g, const void* pts, size_t stride, void* const* dst, size_t count, hipStream_t stream);
hipError_t launch_points_bad_begin(unsigned long long* word, unsigned long long* saved, hipStream_t stream);
hipError_t launch_points_bad_end(unsigned long long* word, const unsigned long long* saved, unsigned long long begin, hipStream_t stream);
// Point-major value and gradient (k_points_grad.hip, points_grad.h): component d of point i goes to grad[i * gstride + d].
// The fused kernels (N = 2, 3: multilinear on the re-laid table, multicubic on the tiled table), and the split path's last
// step, which interleaves ndims component arrays (`src`: host array of device pointers) into the gradient rows.
bool points_grad_fused_applies(const GridDesc& g, size_t stride, size_t gstride);
hipError_t launch_points_grad(const GridDesc& g, const void* pts, size_t stride, void* out, void* grad, size_t gstride, size_t npts,
                              unsigned long long* first_bad, hipStream_t stream);
hipError_t launch_join_grad(const GridDesc& g, const void* const* src, void* grad, size_t gstride, size_t count, hipStream_t stream);
}  // namespace interpn

namespace interpn_abi {

using namespace interpn;

extern std::atomic<int> g_fma;                        // process default of the `fma` flavour (interpn_hip_set_fma)
extern thread_local std::string t_last_hip_error;

int hip_fail(hipError_t e);

#define HIP_TRY(expr)                        \
  do {                                       \
    hipError_t _e = (expr);                  \
    if (_e != hipSuccess) return hip_fail(_e); \
  } while (0)

// Axis length limits of the device kernels (cell indices are 32-bit; f32 classifies cells by
// comparing against (float)n, exact only up to 2^24).
template <typename T> constexpr size_t max_axis_len() { return sizeof(T) == 8 ? (size_t)2147483391u : (size_t)16777216u; }

bool checked_product(const size_t* dims, size_t n, size_t* out);

class DeviceGuard {
 public:
  explicit DeviceGuard(int device) : prev_(-1), ok_(true) {
    if (hipGetDevice(&prev_) != hipSuccess) { ok_ = false; return; }
    if (device >= 0 && device != prev_) {
      if (hipSetDevice(device) != hipSuccess) ok_ = false;
      changed_ = true;
    }
  }
  ~DeviceGuard() {
    if (changed_ && prev_ >= 0) (void)hipSetDevice(prev_);
  }
  bool ok() const { return ok_; }

 private:
  int prev_;
  bool ok_;
  bool changed_ = false;
};

// ---- per-device pool (abi_pool.hip)
hipError_t pool_alloc(int device, void** out, size_t bytes);  // the current device must be `device`
void pool_free(int device, void* p);                          // only for blocks no in-flight work still touches
size_t pool_trim(int device);                                 // frees what the pool holds for `device` (current device = `device`)
hipError_t pool_take_kit(int device, hipStream_t* stream, unsigned long long** flag_host);
void pool_return_kit(int device, hipStream_t stream, unsigned long long* flag_host);
hipError_t pool_take_pinned_word(int device, unsigned long long** word);
void pool_return_pinned_word(int device, unsigned long long* word);
// Staging of the small-batch host path: pinned host memory the kernel reads and writes directly
// over PCIe (zero-copy).  One fixed size serves every interpolator: 8 coordinate arrays + 1 result
// array of kSmallPoints f64 elements.
constexpr size_t kSmallPoints = 8192;
constexpr size_t kSmallBytes = (size_t)(8 + 1) * kSmallPoints * 8;

hipError_t pool_take_small(int device, void** buf);
void pool_return_small(int device, void* buf);
struct DeviceProps { int num_cus = 256, num_xcds = 8; long long l2_bytes = 4 << 20, lds_per_cu = 160 << 10, lds_per_wg = 64 << 10; };
DeviceProps device_props(int device);
int device_num_cus(int device);

// The runtime scratch_slots.h runs on in the product: every member forwards to one hip* call or to the pool.
struct HipRuntime {
  using Stream = hipStream_t;
  using Event = hipEvent_t;
  static constexpr int kNotReady = (int)hipErrorNotReady;
  const int* device = nullptr;  // the handle's (the current device whenever a block is allocated)
  int is_capturing(Stream s, bool* capturing) const {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const hipError_t e = hipStreamIsCapturing(s, &cs);
    *capturing = cs != hipStreamCaptureStatusNone;
    return (int)e;
  }
  int event_create(Event* ev) const { return (int)hipEventCreateWithFlags(ev, hipEventDisableTiming); }
  int event_destroy(Event ev) const { return (int)hipEventDestroy(ev); }
  int event_record(Event ev, Stream s) const { return (int)hipEventRecord(ev, s); }
  int event_query(Event ev) const { return (int)hipEventQuery(ev); }
  int event_synchronize(Event ev) const { return (int)hipEventSynchronize(ev); }
  int stream_wait_event(Stream s, Event ev) const { return (int)hipStreamWaitEvent(s, ev, 0); }
  int stream_synchronize(Stream s) const { return (int)hipStreamSynchronize(s); }
  int device_synchronize() const { return (int)hipDeviceSynchronize(); }
  void clear_last_error() const { (void)hipGetLastError(); }
  int alloc_block(void** out, size_t bytes) const { return (int)pool_alloc(*device, out, bytes); }
  void free_block(void* p) const { pool_free(*device, p); }
};

}  // namespace interpn_abi

struct interpn_hip_interp : scratch_slots::Table<interpn_abi::HipRuntime> {
  interpn::GridDesc desc;
  int device = 0;
  void* vals_owned = nullptr;   // device copy of vals when created from host memory
  void* grids_owned = nullptr;  // one device allocation holding all rectilinear axes
  void* bricks_owned = nullptr; // bricked copy of vals (3-D multilinear f64)
  void* bricks11_owned = nullptr;  // 4-D multicubic: fully overlapped tiles for binned evaluation when `bricks` is another layout
  void* sweep_owned = nullptr;     // 3-D f64 multilinear: the sweep evaluation's table when `bricks` is another layout (desc.sweep_bricks)
  unsigned long long* first_bad = nullptr;  // device word, ~0 = no failure
  unsigned long long* finish_word = nullptr;  // pinned landing word of interpn_hip_finish
  unsigned long long* finish_word_dev = nullptr;  // ... as the device sees it (the status kernel's target), or null
  std::mutex finish_mu;
  std::mutex host_mu;  // host-pointer evaluations on one handle share its two lanes: serialised
  // (marks, sync_device_at_destroy: the caller streams interpn_hip_destroy waits for — scratch_slots.h)
  // Host-evaluation workspace (lazily allocated, reused across calls): two pipeline lanes so
  // that the upload of one chunk overlaps the download of the previous one.
  struct HostLane {
    size_t points = 0;
    void* obs = nullptr;                       // ndims * points elements (device)
    void* out = nullptr;                       // points elements (device)
    unsigned long long* flag_dev = nullptr;    // first failing index of the chunk in flight
    unsigned long long* flag_host = nullptr;   // pinned
    hipStream_t stream = nullptr;
  } lane[2];
  // Small batches skip the staging copies altogether (eval_host_impl): pinned host buffer that
  // the kernel reads the coordinates from and writes the results to, and its device address.
  void* small_host = nullptr;
  void* small_dev = nullptr;
  // Binned evaluation (interpn_host.h): scratch for one slice of sorted points, shared by every
  // evaluation through this handle.  Two streams never work in a block at the same time: a block
  // remembers the stream that used it last, and its event is recorded behind that use only when
  // somebody else needs to know (settle_slot) — another stream that takes the block and waits
  // for the event, or a block about to be freed.
  // Up to kMaxBinSlots blocks, one per stream that evaluates concurrently: an evaluation takes
  // the block its stream used last (stream order alone makes the reuse safe: no event, no
  // command on the stream), else an idle one, else makes a new one (unless told not to
  // allocate), else waits — on the device, through the block's event — for the least recently
  // used one.  `bin_mu` guards the slot list and the
  // per-handle report fields (desc.last_binned, desc.tag of a binned launch); the launches
  // themselves are enqueued outside it.
  // The blocks themselves (BinSlot, bin_mu, bin_slots, bin_uses, scratch_allocs) and the rules are scratch_slots.h's.
  interpn_hip_interp() {
    rt.device = &device;
    word_in_block = &sampling.last_word;
  }
  std::atomic<long long> evals_binned{0}, evals_in_place{0}, evals_sweep{0};
  // The device-side sample in front of automatic sweep launches (abi_sweep.hip; guarded by bin_mu).  Thinning it out
  // (option sweep_probe = 2): the sampling kernel also stores (seq << 1 | coherent) into the pinned word `host`; the host
  // looks at it before the next launch — no synchronisation, a verdict that has not landed yet simply is not known yet.
  struct SweepSampling {
    unsigned long long* host = nullptr;
    unsigned* host_dev = nullptr;  // its device address (null: no host view of the verdicts, every launch is sampled)
    unsigned seq = 0, seen = 0;
    int streak = 0;           // samples in a row that came out unordered
    int streak_coherent = 0;  // ... that came out coherent
    int skipped = 0;          // automatic launches since the last sample
    // the verdict word of the most recent automatic launch's sample, inside a scratch block (option "sweep_probe_took_brick";
    // tests, bench); null when that launch was not sampled or its block has been freed since
    const void* last_word = nullptr;
  } sampling;
};

// A field set (abi_fields.hip, abi_fields_lattice.hip).
struct interpn_hip_fields {
  int device = 0;
  int dtype = interpn::kF64;
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
  int points_path = -1;           // option, point-major form: -1 automatic, 1 fused wherever the table exists, 2 split
  int last_points_path = -1;      // INTERPN_HIP_FIELDS_POINTS_PATH_* of the last point-major call, -1 before any
  int last_lattice_path = -1;     // INTERPN_HIP_FIELDS_LATTICE_PATH_* of the last lattice call, -1 before any
  int last_lattice_group = 0;     // G of the last fused lattice call
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
  // ... and, for interpn_hip_fields_eval_grad_host, its K * N gradient rows (rows of host_grad_points elements)
  void* host_grad = nullptr;
  size_t host_grad_points = 0;
};

namespace interpn {
struct LatticeShape;
struct LatticePlan;
}  // namespace interpn

namespace interpn_abi {

// ---------------------------------------------------------------------------
// Validation, in the order of the reference's `interpn` + `new` (+ `interp`).
// `nobs`/`obs_lens` may be absent (handle creation): pass check_obs = false.
template <typename T>
int validate_regular(int method, const size_t* dims, size_t ndims, const T* starts, size_t nstarts,
                     const T* steps, size_t nsteps, size_t nvals) {
  if (method == kNearest) {
    if (nstarts != ndims || nsteps != ndims) return INTERPN_HIP_ERR_DIM_MISMATCH;  // nearest/regular.rs:50
    if (ndims < 1 || ndims > 6) return INTERPN_HIP_ERR_TOO_MANY_DIMS_6;            // nearest/regular.rs:97
  } else if (method == kLinear) {
    // multilinear/regular.rs:60 — obs.len() is checked by the caller of this helper
    if (nstarts != ndims || nsteps != ndims) return INTERPN_HIP_ERR_DIM_MISMATCH;
    if (ndims < 1 || ndims > 8) return INTERPN_HIP_ERR_TOO_MANY_DIMS;  // regular.rs:111-113
  } else {
    if (ndims < 1 || ndims > 8) return INTERPN_HIP_ERR_TOO_MANY_DIMS;  // multicubic/regular.rs:130-132
    // multicubic/regular.rs:66-73 — try_into().unwrap() panics in the flattened arm
    if (ndims <= 4 && (nstarts != ndims || nsteps != ndims)) return INTERPN_HIP_ERR_REFERENCE_PANIC;
  }
  if (!dims || !starts || !steps) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  size_t prod;
  if (!checked_product(dims, ndims, &prod)) return INTERPN_HIP_ERR_REFERENCE_PANIC;
  if (method == kCubic && !(nstarts == ndims && nsteps == ndims)) return INTERPN_HIP_ERR_DIM_MISMATCH;
  if (nvals != prod) return INTERPN_HIP_ERR_DIM_MISMATCH;  // regular.rs:239 / multicubic/regular.rs:254
  const size_t minlen = method == kCubic ? 4 : 2;
  for (size_t i = 0; i < ndims; ++i)
    if (dims[i] < minlen) return method == kCubic ? INTERPN_HIP_ERR_MIN_FOUR_ENTRIES : INTERPN_HIP_ERR_MIN_TWO_ENTRIES;
  for (size_t i = 0; i < ndims; ++i)
    if (!(steps[i] > (T)0)) return INTERPN_HIP_ERR_NOT_MONOTONIC;  // regular.rs:248
  for (size_t i = 0; i < ndims; ++i)
    if (dims[i] > max_axis_len<T>()) return INTERPN_HIP_ERR_UNSUPPORTED;
  return INTERPN_HIP_OK;
}

template <typename T>
int validate_rectilinear(int method, const T* const* grids, const size_t* grid_lens, size_t ngrids, size_t nvals) {
  const size_t ndims = ngrids;
  if (method == kNearest) {
    if (ndims < 1 || ndims > 6) return INTERPN_HIP_ERR_TOO_MANY_DIMS_6;  // nearest/rectilinear.rs:59
  } else if (ndims < 1 || ndims > 8) return INTERPN_HIP_ERR_TOO_MANY_DIMS;  // rectilinear.rs:77-79
  if (!grids || !grid_lens) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
  size_t prod;
  if (!checked_product(grid_lens, ndims, &prod)) return INTERPN_HIP_ERR_REFERENCE_PANIC;
  if (nvals != prod) return INTERPN_HIP_ERR_DIM_MISMATCH;  // rectilinear.rs:186 / multicubic/rectilinear.rs:208
  const size_t minlen = method == kCubic ? 4 : 2;
  for (size_t i = 0; i < ndims; ++i)
    if (grid_lens[i] < minlen) return method == kCubic ? INTERPN_HIP_ERR_MIN_4_ENTRIES : INTERPN_HIP_ERR_MIN_2_ENTRIES;
  for (size_t i = 0; i < ndims; ++i) {
    if (!grids[i]) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
    if (!(grids[i][1] > grids[i][0])) return INTERPN_HIP_ERR_NOT_MONOTONIC;  // rectilinear.rs:195
  }
  for (size_t i = 0; i < ndims; ++i)
    if (grid_lens[i] > max_axis_len<T>()) return INTERPN_HIP_ERR_UNSUPPORTED;
  return INTERPN_HIP_OK;
}

// `.interp(obs, out)` length checks (multilinear/regular.rs:271, multicubic/regular.rs:301, ...),
// including the flattened cubic arms' `obs.try_into().unwrap()` panic.
inline int validate_obs(const GridDesc& g, const size_t* obs_lens, size_t nobs, size_t nout) {
  const size_t ndims = (size_t)g.ndims;
  if (is_one_dim(g.method)) {  // Interp1D::eval(locs, out), one_dim/mod.rs:52-54: one coordinate array
    if (nobs != 1) return INTERPN_HIP_ERR_INVALID_ARGUMENT;
    if (obs_lens && obs_lens[0] != nout) return INTERPN_HIP_ERR_LENGTH_MISMATCH;
    return INTERPN_HIP_OK;
  }
  if (nobs != ndims) {
    if (g.method == kCubic && ndims <= 4) return INTERPN_HIP_ERR_REFERENCE_PANIC;
    return INTERPN_HIP_ERR_DIM_MISMATCH;
  }
  if (obs_lens)
    for (size_t i = 0; i < ndims; ++i)
      if (obs_lens[i] != nout) return INTERPN_HIP_ERR_DIM_MISMATCH;
  return INTERPN_HIP_OK;
}

int resolve_device(int device, int* out);

// abi_layout.hip
int maybe_build_bricks(interpn_hip_interp* h);

// abi_options.hip
bool option_access(LaunchConfig& c, const char* name, long long* value, bool set);
void latch_env(LaunchConfig& c);

// abi_create.hip
// Set by the field-set creators (abi_fields.hip) around the creation of their per-field handles: finish_create then
// leaves the re-laid table out, and maybe_build_bricks is called when the per-field path is first used.
extern thread_local bool t_defer_tables;
int finish_create(interpn_hip_interp* h, const void* vals, size_t nvals, size_t elem, int vals_mem);
template <typename T>
int create_regular(int method, const size_t* dims, size_t ndims, const T* starts, size_t nstarts, const T* steps,
                   size_t nsteps, const T* vals, size_t nvals, int vals_mem, int linearize, int device,
                   interpn_hip_interp** handle);
template <typename T>
int create_rectilinear(int method, const T* const* grids, const size_t* grid_lens, size_t ngrids, const T* vals,
                       size_t nvals, int vals_mem, int linearize, int device, interpn_hip_interp** handle);
template <typename T>
int create_one_dim(int method, int kind, T start, T step, const T* grid, size_t ngrid, const T* vals, size_t nvals,
                   int vals_mem, int device, interpn_hip_interp** handle);

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Whether `stream` is being captured into a graph; a failed query counts as captured (nothing is allocated or waited for).
inline bool stream_capturing(hipStream_t stream) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &cs) != hipSuccess) { (void)hipGetLastError(); return true; }
  return cs != hipStreamCaptureStatusNone;
}

// The status of a sequence of launches through `h` that failed half-way: part of it may be in flight without a stream mark
// behind it, so interpn_hip_destroy synchronises the device.
inline int fail_sequence(interpn_hip_interp* h, hipError_t err, int st) {
  (void)hipGetLastError();
  std::lock_guard<std::mutex> lk(h->marks_mu);
  h->sync_device_at_destroy = true;
  return err != hipSuccess ? hip_fail(err) : st;
}

// abi_launch.hip
hipError_t launch_any(const GridDesc& g, const void* const* obs, void* out, size_t npts,
                      unsigned long long* first_bad, hipStream_t stream);
void mark_stream(interpn_hip_interp* h, hipStream_t stream);
// Chunk size of the host pipeline (points).  Bounded so that the workspace stays modest
// (8 dims x 8 B x 4 Mi = 256 MiB worst case) while each kernel launch still fills the chip.
constexpr size_t kHostChunkPoints = (size_t)4 << 20;

// abi_host.hip: what interpn_hip_finish does, for the first-failing-index words of `count` handles whose work is on `s`
// (`h` lends its pinned word): ONE command behind that work brings the smallest of the words to the host, the stream is
// synchronised, and — only when a point failed — every word is reset.  Returns a status, or -1 when the words cannot travel
// together (more than kMaxStatusWords of them, a stream under capture, no device view of the pinned word, option
// finish_kernel = 0) and count > 1: the caller then asks handle by handle.  One word travels by the status kernel too, or
// by an 8-byte copy where the kernel cannot be used.
constexpr int kMaxStatusWords = 32;
int finish_words(interpn_hip_interp* h, hipStream_t s, unsigned long long* const* words, int count, uint64_t* first_bad_index);

// abi_binned.hip
int binned_applies(const GridDesc& g, size_t npoints);
interpn_hip_interp::BinSlot* take_bin_slot(interpn_hip_interp* h, size_t need, hipStream_t stream, bool may_alloc, int* why);
void release_bin_slot(interpn_hip_interp* h, interpn_hip_interp::BinSlot* slot, hipStream_t stream, bool staged);
// (bin_mu held) Makes the block's last use known to the runtime: records the block's event on the stream of that use, which
// covers everything that stream holds by now.  Afterwards `recorded` says whether there is an event to wait for (none: the
// block was never used, or its stream is gone and the device has been waited for instead).  False: that stream is being
// captured and must not be touched — the block cannot be handed to anybody else right now.
bool settle_slot(interpn_hip_interp* h, interpn_hip_interp::BinSlot& slot);

// abi_lattice.hip: scratch blocks of the paths that fill one themselves and hand it to interpn_hip_eval_device_ex (the
// lattice's expanded path, the point-major split path).  Under graph capture a block is taken without touching any event;
// claim_slot drops what the sort and the sweep remembered about the block's contents; reserve_slots makes sure
// `nstreams` blocks of at least `need` bytes exist (the current device is the handle's).
interpn_hip_interp::BinSlot* take_slot_captured(interpn_hip_interp* h, size_t need, hipStream_t stream);
void release_slot_captured(interpn_hip_interp* h, interpn_hip_interp::BinSlot* slot);
void claim_slot(interpn_hip_interp* h, interpn_hip_interp::BinSlot* slot);
int reserve_slots(interpn_hip_interp* h, size_t need, int nstreams);
// ... and what the lattice forms of a field set (abi_fields_lattice.hip) share with the single handle's: the shape of a
// lattice from the caller's arrays, the checks every lattice entry point makes (in this order; *empty: some axis has no
// coordinates), the scratch one evaluation needs on the path `plan` names, the larger of the two paths' needs (reserve),
// and one lattice on device arrays through the handle.
// (`*indexable`: the grid's values are indexed with 32 bits; `n`: the grid's axis lengths as the plans take them) the
// argument checks the two plan entry points share.
int lattice_plan_args(size_t elem_size, int method, size_t ndims, const size_t* dims, const size_t* axis_lens, int* n,
                      interpn::LatticeShape* s, bool* indexable);
int lattice_make_shape(const void* const* axes, const size_t* axis_lens, size_t naxes, interpn::LatticeShape* s);
int validate_lattice(const interpn_hip_interp* h, const void* const* axes, const size_t* axis_lens, size_t naxes, const void* out,
                     interpn::LatticeShape* s, bool* empty);
interpn::LatticePlan lattice_plan_for(const GridDesc& g, const interpn::LatticeShape& s);
size_t lattice_scratch_need(const GridDesc& g, const interpn::LatticeShape& s, const interpn::LatticePlan& p);
size_t lattice_reserve_need(const GridDesc& g, const interpn::LatticeShape& s);
size_t lattice_expand_slice(const GridDesc& g, size_t npoints);
int lattice_device(interpn_hip_interp* h, const interpn::LatticeShape& s, void* out, hipStream_t stream, unsigned flags, int* path_taken);
// abi_lattice_grad.hip: the same with the gradient (`grad`: host array of ndims device pointers)
int lattice_grad_device(interpn_hip_interp* h, const interpn::LatticeShape& s, void* out, void* const* grad, hipStream_t stream,
                        unsigned flags, int* path_taken);
constexpr size_t kExpandSliceBytes = (size_t)64 << 20;  // coordinates of one slice (bounds the scratch block)
constexpr size_t kExpandSliceMin = (size_t)1 << 16;     // ... but never fewer points than this

// abi_fields.hip
int ensure_sub_tables(interpn_hip_fields* s);

// abi_fields_grad.hip: whether the column form's value-and-Jacobian evaluation runs its fused kernel (option "fused" and
// its rule) — the point-major split path (abi_fields_points_grad.hip) parks one status word or all K by it
bool grad_takes_fused(const interpn_hip_fields* s);

// abi_grad.hip: the column form's gradient launch, k_linear_grad / k_cubic_grad or the runtime-N kernels by the handle's
// method and each launcher's own rule (also the middle step of the point-major split path, abi_points.hip)
hipError_t launch_grad(const GridDesc& g, const void* const* obs, void* out, void* const* grad, size_t npts,
                       unsigned long long* first_bad, hipStream_t stream);

// abi_sweep.hip
int eval_device_sweep(interpn_hip_interp* h, const void* const* obs, void* out, size_t npoints, hipStream_t stream,
                      unsigned flags, int* why);

// abi_host.hip
int ensure_lane(interpn_hip_interp* h, int which, size_t points);
int eval_host_impl(interpn_hip_interp* h, const void* const* obs, size_t nobs, void* out, size_t nout, size_t* bad_index);

}  // namespace interpn_abi
