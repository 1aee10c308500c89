/*
 * interpn_hip.h — C ABI of libinterpn_hip.so: MI355X (gfx950) implementation of the batched
 * per-observation-point hot path of jlogan03/interpn v0.8.2.
 *
 * What it replaces (paths relative to the reference repository):
 *   multilinear::regular::interpn       src/multilinear/regular.rs:51-117
 *   multilinear::rectilinear::interpn   src/multilinear/rectilinear.rs:49-83
 *   multicubic::regular::interpn        src/multicubic/regular.rs:52-136
 *   multicubic::rectilinear::interpn    src/multicubic/rectilinear.rs:54-104
 * and who would call it: the bodies of the PyO3 functions interpn_{linear,cubic}_
 * {regular,rectilinear}_{f64,f32} (src/python.rs:55-85, 119-147, 228-292) through a Rust
 * `hip_sys` extern block (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - Every Rust slice `&[T]` crosses the boundary as (pointer, length); a slice of slices
 *     `&[&[T]]` as (array of pointers, array of lengths, count).  All buffers are borrowed for
 *     the duration of the call only; nothing is retained after a function returns, except the
 *     device copies a handle owns (and a device `vals` buffer lent with INTERPN_HIP_MEM_DEVICE,
 *     which must outlive the handle).
 *   - `vals` is C-ordered; `obs` is struct-of-arrays (one array per dimension); `out` has one
 *     element per observation point and is written only in [0, nout).
 *   - Return value: 0 on success, otherwise an interpn_hip_status.  interpn_hip_strerror()
 *     returns, for the statuses that mirror a reference error, the reference's exact
 *     `&'static str` (what src/python.rs turns into AssertionError(msg)).
 *   - INTERPN_HIP_ERR_UNREPRESENTABLE ("Unrepresentable coordinate value"): the reference
 *     aborts the batch at the first failing point i with out[0..i) written and out[i..]
 *     untouched.  The host-pointer entry points reproduce exactly that.  The device-pointer
 *     entry point reports i through interpn_hip_finish(); device `out[i..]` is unspecified.
 *   - Conditions on which the reference *panics* (mismatched slice lengths in
 *     multicubic::*::interpn, usize overflow) return INTERPN_HIP_ERR_REFERENCE_PANIC instead
 *     of aborting the process.
 *   - Numerics follow the reference's `fma` cargo feature ON (what every published wheel is
 *     built with, pyproject.toml:72); interpn_hip_set_fma(0) selects the non-fused flavour
 *     (plain `cargo test`).  Results are bit-identical to the Rust code of the same flavour.
 *   - Memory: besides the C-ordered `vals`, a handle may keep a second, re-laid copy of the grid
 *     (cache-line bricks for multilinear N = 2..6, 4 x 4 tiles for multicubic N = 2..4; up to 16x
 *     the grid, bounded by a quarter of the free device memory).  Tuning / testing knobs.  The
 *     environment is read ONCE PER HANDLE, when it is created (never on the launch path); the
 *     per-handle options can be changed afterwards with interpn_hip_set_option(h, "<name>", v),
 *     <name> = the variable's suffix in lower case:
 *       INTERPN_HIP_BRICKS=off|11|12|22|c4|j4 (linear) |44|24|22|14|11 (cubic)   force / disable a layout (creation only;
 *                                       c4 = 4-D cell bricks, j4 = the f32-only 2 x 4 x 4 bricks)
 *       INTERPN_HIP_BLOCKS_PER_CU=n     workgroups per CU a persistent launch grid is sized for (default 8)
 *       INTERPN_HIP_ITERS_PER_BLOCK=n   256-lane rows per workgroup of the one-pass brick kernels (0 = default)
 *       INTERPN_HIP_PPL=1               one point per lane in the multilinear brick kernels (0 = auto)
 *       INTERPN_HIP_FORCE_GENERIC=1     route every evaluation through the runtime-N kernel
 *       INTERPN_HIP_GENERIC_RUNTIME=1   recursive arms: runtime-N form
 *       INTERPN_HIP_GENERIC_VEC=0|1     recursive arms: one-tree / row-vector form (-1 = auto; the
 *                                       row-vector form exists only where it compiles without
 *                                       AGPR or scratch spills, see k_generic.hip)
 *       INTERPN_HIP_AXIS_REGS=0|1|2     rectilinear axes <= 64 coordinates: 0 = search in LDS,
 *                                       1 = across lanes without the lane table, 2 = with it (-1 = auto)
 *       INTERPN_HIP_AXIS_LDS_KB=n       LDS budget of the rectilinear axis image (-1 = default)
 *       INTERPN_HIP_PERSISTENT=1        C-order regular / nearest kernels: persistent grid
 *       INTERPN_HIP_HOST_CHUNK=n        points per chunk of the host-pointer pipeline (0 = default 2 Mi)
 *       INTERPN_HIP_BINNED=-1|0|1       tiled multicubic, device-pointer evaluation: sort the points by table position
 *                                       first (auto: large 4-D batches; 1: always, N = 2..4; 0: never)
 *       INTERPN_HIP_COLUMN=-1|0|1       sorted 4-D multicubic on a regular grid: evaluate out of an LDS-resident table
 *                                       column (auto: from ~3000 points per bin; 1: wherever it applies; 0: never);
 *                                       INTERPN_HIP_COLUMN_THREADS=256|384|768, INTERPN_HIP_COLUMN_PART=n (points per part at most),
 *                                       INTERPN_HIP_COLUMN_GROUPS=1|2, INTERPN_HIP_COLUMN_CPP=n (dim-2 classes per K-range phase),
 *                                       INTERPN_HIP_COLUMN_COEF=0 (every node from the table values; default 1: dim 0 from
 *                                       per-part Hermite coefficients, cubic_column.h), INTERPN_HIP_COLUMN_PAD=-1|0|1 (LDS tiles
 *                                       bare / 16 bytes apart), INTERPN_HIP_COLUMN_TAIL=0xDV (the last 1/D of the bins cut V
 *                                       times finer; default 0x84), INTERPN_HIP_COLUMN_KEYS=0 (regular grids: the local sort's keys
 *                                       from the records instead of from the upper eight bits of the index words, where the sort
 *                                       leaves them by default — slices are then 2^24 points at most),
 *                                       INTERPN_HIP_SCATTER_STAGED=0 (the sort stores records directly)
 *       INTERPN_HIP_SWEEP=-1|0|1        2-D / 3-D multilinear, nearest-neighbour and multicubic (f64, f32), device-pointer evaluation: the sweep kernel (every wave orders 1024 / 1536
 *                                       points by leading cell index on chip, all waves walk the one-line brick table in step
 *                                       with a clock; linear_sweep.h; multicubic: 512 / 1280 points by their cell along dim 2,
 *                                       rows on the fully overlapped tile table, cubic_sweep.h): auto (multilinear: batches of >= 4
 *                                       rounds per wave ~ 1.26e7 points in f64, 8 where the L2 holds the table, f32 3 / 6; multicubic:
 *                                       regular grids with that table beyond the L2, from 2 rounds per wave ~ 4e6 points; 2-D
 *                                       multicubic: f64 regular grids from 8 rounds per wave ~ 2.2e7 points), never,
 *                                       or whenever the handle has the table (creation: 0 also skips building it);
 *                                       INTERPN_HIP_SWEEP_PERIOD=n ticks of 10 ns per sweep (0 = what the previous launch
 *                                       measured, 1 = no clock); INTERPN_HIP_SWEEP_LAYOUT=11|12 (creation only, 3-D f64
 *                                       multilinear: the sweep kernel's table with one line per cell / 1.5 lines per cell at half
 *                                       the size; default: by the table's size against the points an XCD holds per sweep)
 *       INTERPN_HIP_FINISH_KERNEL=1|0   interpn_hip_finish / interpn_hip_fields_finish: how the 8-byte status word reaches the host.
 *                                       1 (default): a one-lane kernel behind the evaluations on the stream stores it into pinned
 *                                       memory (a field set's K words travel as their minimum: one command, one wait).  0: an
 *                                       8-byte hipMemcpyAsync per handle; a stream under capture always takes the copy.  Either
 *                                       way finish then calls hipStreamSynchronize: when it returns, everything enqueued on
 *                                       `stream` before the call is complete for the device and for the HIP runtime — results may
 *                                       be consumed on any stream, and an event recorded before the call reads complete
 *       INTERPN_HIP_BIN_SLICE_LOG2=n    log2 of the points sorted per slice (16..27, default 25): bounds a scratch block
 *       INTERPN_HIP_AXIS_RECORDS=0      rectilinear multilinear: search with coordinates + tables, not per-bucket records
 *       INTERPN_HIP_CUBIC_RECORDS=n     rectilinear multicubic (creation only): per-cell records of the axes (cubic_cell_record.h: a
 *                                       dimension's setup without divisions) while they take at most n KiB (default 40; 0: never —
 *                                       the kernels then do the setup's divisions per point)
 *       INTERPN_HIP_BIN_SCRAMBLE=1      testing: the sort misplaces every 5th point by one bin (results must not change)
 *       options without an environment variable: "fma" (the handle's flavour), "stage_timing" (interpn_hip_stage_ms),
 *                                       "debug_stamps" + "debug_stamps_bytes" (address and size of a device buffer for the column
 *                                       kernel's time stamps, 64 bytes per part; a launch that needs more writes none)
 *       INTERPN_HIP_POOL_MB=n           device bytes of destroyed handles kept for reuse, per device
 *                                       (process-wide, read once; default 1024; 0 = release
 *                                       everything at destroy)
 *   - Thread safety: all functions are re-entrant.  Device-pointer evaluations on one handle may
 *     run concurrently (the grid is read-only; the sticky first-bad-index word of the handle is
 *     shared by them); host-pointer evaluations on one handle share its staging buffers and are
 *     serialised internally — use one handle per thread to overlap them.
 */
#ifndef INTERPN_HIP_H
#define INTERPN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum interpn_hip_status {
  INTERPN_HIP_OK = 0,
  /* mirrors of the reference's error strings */
  INTERPN_HIP_ERR_DIM_MISMATCH = 1,      /* "Dimension mismatch" */
  INTERPN_HIP_ERR_MIN_TWO_ENTRIES = 2,   /* "All grids must have at least two entries"  multilinear/regular.rs:245 */
  INTERPN_HIP_ERR_MIN_2_ENTRIES = 3,     /* "All grids must have at least 2 entries"    multilinear/rectilinear.rs:192 */
  INTERPN_HIP_ERR_MIN_FOUR_ENTRIES = 4,  /* "All grids must have at least four entries" multicubic/regular.rs:261 */
  INTERPN_HIP_ERR_MIN_4_ENTRIES = 5,     /* "All grids must have at least 4 entries"    multicubic/rectilinear.rs:214 */
  INTERPN_HIP_ERR_NOT_MONOTONIC = 6,     /* "All grids must be monotonically increasing" */
  INTERPN_HIP_ERR_UNREPRESENTABLE = 7,   /* "Unrepresentable coordinate value"          multilinear/regular.rs:418 */
  INTERPN_HIP_ERR_TOO_MANY_DIMS = 8,     /* "Dimension exceeds maximum (8). Use interpolator struct directly for higher dimensions." */
  INTERPN_HIP_ERR_REFERENCE_PANIC = 9,   /* the reference would panic here */
  INTERPN_HIP_ERR_TOO_MANY_DIMS_6 = 10,  /* "Dimension exceeds maximum (6)."           nearest/regular.rs:97 */
  INTERPN_HIP_ERR_LENGTH_MISMATCH = 11,  /* "Length mismatch"                           one_dim/mod.rs:53, :150 */
  INTERPN_HIP_ERR_UNREPRESENTABLE_NUMBER = 12, /* "Unrepresentable number"              one_dim/mod.rs:111 */
  /* statuses of this implementation */
  INTERPN_HIP_ERR_INVALID_ARGUMENT = 32, /* null pointer, unknown enum value, dtype mismatch */
  INTERPN_HIP_ERR_UNSUPPORTED = 33,      /* axis longer than 2^31-257 points (f32: 2^24); interpn_hip_eval_grad_* on a handle
                                            that is not multilinear (multicubic, nearest, interpn::one_dim);
                                            interpn_hip_eval_cubic_grad_* on a handle that is not multicubic */
  INTERPN_HIP_ERR_NO_DEVICE = 34,        /* no usable HIP device */
  INTERPN_HIP_ERR_OUT_OF_MEMORY = 35,    /* device or pinned-host allocation failed */
  INTERPN_HIP_ERR_HIP = 36               /* any other HIP runtime failure (see interpn_hip_last_hip_error) */
} interpn_hip_status;

enum { INTERPN_HIP_LINEAR = 0, INTERPN_HIP_CUBIC = 1, INTERPN_HIP_NEAREST = 2 }; /* method */
/* The reference's `fma` cargo feature (Cargo.toml:34-38) is a PER-INTERPOLATOR property here: OR one
 * of these into the `method` argument of interpn_hip_create_* (neither = the process default, see
 * interpn_hip_set_fma).  Handles of both flavours can be evaluated concurrently from different
 * threads.  Also readable / writable as the per-handle option "fma" (not while evaluations of the
 * same handle are being enqueued by another thread). */
enum { INTERPN_HIP_FLAVOUR_FMA = 0x100, INTERPN_HIP_FLAVOUR_NO_FMA = 0x200 };
/* interpn::one_dim (src/one_dim/), for interpn_hip_create_grid1d_* only; the flavour bits OR into them as above. */
enum {
  INTERPN_HIP_LINEAR_1D = 16,           /* one_dim::linear::Linear1D          one_dim/linear.rs:26-37 */
  INTERPN_HIP_LINEAR_HOLD_LAST_1D = 17, /* one_dim::linear::LinearHoldLast1D  one_dim/linear.rs:60-85 */
  INTERPN_HIP_LEFT_1D = 18,             /* one_dim::hold::Left1D              one_dim/hold.rs:26-38 */
  INTERPN_HIP_RIGHT_1D = 19,            /* one_dim::hold::Right1D             one_dim/hold.rs:61-73 */
  INTERPN_HIP_NEAREST_1D = 20           /* one_dim::hold::Nearest1D           one_dim/hold.rs:94-107 */
};
enum { INTERPN_HIP_MEM_HOST = 0, INTERPN_HIP_MEM_DEVICE = 1 }; /* where a buffer lives */

const char* interpn_hip_strerror(int status);
/* Text of the last HIP runtime error seen by the calling thread ("" if none). */
const char* interpn_hip_last_hip_error(void);
/* Library version "major.minor.patch". */
const char* interpn_hip_version(void);
/* DEPRECATED default-setter, kept for the one-shot entry points (whose signatures are the Rust
 * functions' and have no place for a flavour — there it plays the role of the compile-time cargo
 * feature): flavour of interpolators created afterwards WITHOUT an INTERPN_HIP_FLAVOUR_* flag
 * (process-wide; default 1).  Returns the previous value.  Never changes an existing handle. */
int interpn_hip_set_fma(int enabled);
/* Number of visible HIP devices (0 when none; never fails). */
int interpn_hip_device_count(void);
/* Give back to the driver the device memory of destroyed handles that the library keeps for reuse
 * on `device` (-1: the current device): cached and parked blocks alike (INTERPN_HIP_POOL_MB).
 * Waits for the device like hipFree.  *freed_bytes (may be NULL) receives what was released. */
int interpn_hip_trim(int device, size_t* freed_bytes);

/* ------------------------------------------------------------------------------------------
 * One-shot entry points, host pointers — drop-in for the calls made inside the PyO3 bodies.
 * They build the interpolator, move the batch through the current HIP device in chunks and
 * return when `out` is complete.
 *
 * interpn_hip_linear_regular_*      <- multilinear::regular::interpn(dims, starts, steps, vals, obs, out)
 *                                      src/python.rs:69-76
 * interpn_hip_linear_rectilinear_*  <- multilinear::rectilinear::interpn(grids, vals, obs, out)
 *                                      src/python.rs:133-138
 * interpn_hip_cubic_regular_*       <- multicubic::regular::interpn(dims, starts, steps, vals,
 *                                      linearize_extrapolation, obs, out)  src/python.rs:243-251
 * interpn_hip_cubic_rectilinear_*   <- multicubic::rectilinear::interpn(grids, vals,
 *                                      linearize_extrapolation, obs, out)  src/python.rs:277-283
 * interpn_hip_nearest_regular_*     <- nearest::regular::interpn(dims, starts, steps, vals, obs, out)
 *                                      src/python.rs:162-169   (N <= 6)
 * interpn_hip_nearest_rectilinear_* <- nearest::rectilinear::interpn(grids, vals, obs, out)
 *                                      src/python.rs:192
 * ---------------------------------------------------------------------------------------- */
#define INTERPN_HIP_DECLARE_ONESHOT(T, SUFFIX)                                                            \
  int interpn_hip_linear_regular_##SUFFIX(const size_t* dims, size_t ndims, const T* starts,             \
                                          size_t nstarts, const T* steps, size_t nsteps, const T* vals,  \
                                          size_t nvals, const T* const* obs, const size_t* obs_lens,     \
                                          size_t nobs, T* out, size_t nout);                             \
  int interpn_hip_linear_rectilinear_##SUFFIX(const T* const* grids, const size_t* grid_lens,            \
                                              size_t ngrids, const T* vals, size_t nvals,                \
                                              const T* const* obs, const size_t* obs_lens, size_t nobs,  \
                                              T* out, size_t nout);                                      \
  int interpn_hip_cubic_regular_##SUFFIX(const size_t* dims, size_t ndims, const T* starts,              \
                                         size_t nstarts, const T* steps, size_t nsteps, const T* vals,   \
                                         size_t nvals, int linearize_extrapolation, const T* const* obs, \
                                         const size_t* obs_lens, size_t nobs, T* out, size_t nout);      \
  int interpn_hip_cubic_rectilinear_##SUFFIX(const T* const* grids, const size_t* grid_lens,             \
                                             size_t ngrids, const T* vals, size_t nvals,                 \
                                             int linearize_extrapolation, const T* const* obs,           \
                                             const size_t* obs_lens, size_t nobs, T* out, size_t nout);      \
  int interpn_hip_nearest_regular_##SUFFIX(const size_t* dims, size_t ndims, const T* starts,            \
                                           size_t nstarts, const T* steps, size_t nsteps, const T* vals, \
                                           size_t nvals, const T* const* obs, const size_t* obs_lens,    \
                                           size_t nobs, T* out, size_t nout);                            \
  int interpn_hip_nearest_rectilinear_##SUFFIX(const T* const* grids, const size_t* grid_lens,           \
                                               size_t ngrids, const T* vals, size_t nvals,               \
                                               const T* const* obs, const size_t* obs_lens, size_t nobs, \
                                               T* out, size_t nout);

INTERPN_HIP_DECLARE_ONESHOT(double, f64)
INTERPN_HIP_DECLARE_ONESHOT(float, f32)

/* ------------------------------------------------------------------------------------------
 * Persistent interpolators — the counterpart of MultilinearRegular::new / MulticubicRegular::new
 * ... (src/multilinear/regular.rs:225-259, rectilinear.rs:175-201, multicubic/regular.rs:239-288,
 * rectilinear.rs:193-228) whose grid stays resident in HBM between evaluations, and of
 * `.interp(obs, out)` (regular.rs:268-283 etc.).  This is the surface the Python classes'
 * `.eval()` sits on (src/interpn/multilinear_regular.py:101-168).
 *
 * `method`  INTERPN_HIP_LINEAR | INTERPN_HIP_CUBIC | INTERPN_HIP_NEAREST
 * `vals_mem` INTERPN_HIP_MEM_HOST: `vals` is copied to the device;
 *            INTERPN_HIP_MEM_DEVICE: `vals` is a device pointer on `device`, borrowed (e.g. the
 *            buffer an RCCL broadcast just filled on this rank).
 * `device`  HIP device ordinal, or -1 for the calling thread's current device.
 * Validation (order and messages) is the reference's `new`.  Axis coordinates, starts and steps
 * are always host pointers (they are a few KiB).
 * ---------------------------------------------------------------------------------------- */
typedef struct interpn_hip_interp interpn_hip_interp;

#define INTERPN_HIP_DECLARE_CREATE(T, SUFFIX)                                                             \
  int interpn_hip_create_regular_##SUFFIX(int method, const size_t* dims, size_t ndims, const T* starts, \
                                          size_t nstarts, const T* steps, size_t nsteps, const T* vals,  \
                                          size_t nvals, int vals_mem, int linearize_extrapolation,       \
                                          int device, interpn_hip_interp** handle);                      \
  int interpn_hip_create_rectilinear_##SUFFIX(int method, const T* const* grids,                         \
                                              const size_t* grid_lens, size_t ngrids, const T* vals,     \
                                              size_t nvals, int vals_mem, int linearize_extrapolation,   \
                                              int device, interpn_hip_interp** handle);

INTERPN_HIP_DECLARE_CREATE(double, f64)
INTERPN_HIP_DECLARE_CREATE(float, f32)

/* ------------------------------------------------------------------------------------------
 * interpn::one_dim — the counterpart of RegularGrid1D::new(start, step, vals) (one_dim/mod.rs:86-95) or
 * RectilinearGrid1D::new(grid, vals) (one_dim/mod.rs:148-154) wrapped in one of the five interpolators
 * (`method` = INTERPN_HIP_*_1D [| INTERPN_HIP_FLAVOUR_*]).  Every check runs before any device work:
 *   regular      nvals < 2: INTERPN_HIP_ERR_REFERENCE_PANIC (the reference panics at the first evaluated point, or in
 *                `new` for an empty slice); no check of `step` (zero, negative, NaN are accepted);
 *                stop = start + step * T(nvals - 1), two roundings in T
 *   rectilinear  ngrid != nvals or ngrid < 2: INTERPN_HIP_ERR_LENGTH_MISMATCH; no sortedness check
 *   both         more than 2^31 - 257 values, or a rectilinear axis of 4 GiB or more (f64: 2^29 values, f32: 2^30):
 *                INTERPN_HIP_ERR_UNSUPPORTED
 * The handle has ndims = 1 and is evaluated by the existing entry points (eval_host, eval_device(_ex), the sharded
 * forms, finish, replicate), which mirror Interp1D::eval (one_dim/mod.rs:51-61): nobs != 1 is
 * INTERPN_HIP_ERR_INVALID_ARGUMENT, obs_lens[0] != nout INTERPN_HIP_ERR_LENGTH_MISMATCH, and a point whose cell index
 * does not convert to isize (regular grids: NaN, +-inf, |(x - start) / step| >= 2^63) is
 * INTERPN_HIP_ERR_UNREPRESENTABLE_NUMBER with the abort-at-first-bad-point contract described above (where the other
 * handles say INTERPN_HIP_ERR_UNREPRESENTABLE).  Rectilinear grids never fail a point.  interpn_hip_check_bounds_device
 * returns INTERPN_HIP_ERR_INVALID_ARGUMENT (the reference has no bounds check for one_dim); interpn_hip_table_bytes
 * reports the per-cell record table (k_one_dim.hip).
 * ---------------------------------------------------------------------------------------- */
#define INTERPN_HIP_DECLARE_CREATE_1D(T, SUFFIX)                                                                  \
  int interpn_hip_create_grid1d_regular_##SUFFIX(int method, T start, T step, const T* vals, size_t nvals,        \
                                                 int vals_mem, int device, interpn_hip_interp** handle);          \
  int interpn_hip_create_grid1d_rectilinear_##SUFFIX(int method, const T* grid, size_t ngrid, const T* vals,      \
                                                     size_t nvals, int vals_mem, int device,                      \
                                                     interpn_hip_interp** handle);

INTERPN_HIP_DECLARE_CREATE_1D(double, f64)
INTERPN_HIP_DECLARE_CREATE_1D(float, f32)

/* Clone `src` onto `device` (-1 = current) of the same process: the grid (and the axes of a
 * rectilinear grid) travels device to device (hipMemcpyPeer, i.e. xGMI between the GPUs of one
 * node; no host staging, no second upload), the re-laid table is rebuilt on the target.  The
 * single-process way to "replicate the read-only grid on every GPU"  in
 * front of interpn_hip_eval_host_sharded; multi-process callers broadcast `vals` with RCCL and
 * create from the device pointer (INTERPN_HIP_MEM_DEVICE).  The clone owns its copy. */
int interpn_hip_replicate(const interpn_hip_interp* src, int device, interpn_hip_interp** out);

/* sizeof of the element type of the interpolator (8 or 4), number of dimensions, device. */
int interpn_hip_elem_size(const interpn_hip_interp* h);
int interpn_hip_ndims(const interpn_hip_interp* h);
int interpn_hip_device(const interpn_hip_interp* h);

/* Evaluate on host arrays (synchronous).  `obs`/`out` element type must be the handle's.
 * Mirrors `.interp(obs, out)`: "Dimension mismatch" unless nobs == ndims and every
 * obs_lens[d] == nout; abort-at-first-bad-point semantics as described above. */
int interpn_hip_eval_host(interpn_hip_interp* h, const void* const* obs, const size_t* obs_lens,
                          size_t nobs, void* out, size_t nout);

/* Single-process multi-GPU form of `interpn_hip_eval_host`: cuts the observation index into
 * `nhandles` contiguous ranges (the first nout % nhandles ranges one point longer; SURVEY.md
 * section 8(e)) and evaluates range r with handles[r] on that handle's device, one host thread per
 * handle, no device-to-device traffic.  The handles must be distinct and describe the same
 * interpolator (create one per device from the same grid).  Status and checks as
 * `interpn_hip_eval_host`.  On INTERPN_HIP_ERR_UNREPRESENTABLE `*first_bad_index` (optional)
 * receives the global index i of the first failing point; out[0..i) holds the reference's
 * results, out[i..] is unspecified here (ranges behind the failing one ran concurrently),
 * where the one-handle form leaves it untouched. */
int interpn_hip_eval_host_sharded(interpn_hip_interp* const* handles, size_t nhandles,
                                  const void* const* obs, const size_t* obs_lens, size_t nobs,
                                  void* out, size_t nout, uint64_t* first_bad_index);

/* Device-resident single-process multi-GPU form (round 4): a caller that is ONE process — the
 * reference's PyO3 module is (src/python.rs:58-80) — with the observation points already sharded
 * over the devices.  Shard r is obs[r][0..nobs) (a HOST array of `nobs` DEVICE pointers on the
 * device of handles[r], each to npoints[r] elements) -> out[r] (a device pointer there), enqueued
 * on streams[r] (hipStream_t; `streams` or an entry may be NULL = default stream).  All shards
 * are enqueued before the first one is waited for; the call returns when every shard has finished.
 * No PCIe traffic besides the 8-byte status words, no collective.  The handles must be distinct
 * and describe the same interpolator (interpn_hip_replicate).  On
 * INTERPN_HIP_ERR_UNREPRESENTABLE `*first_bad_index` (optional) is the global index of the
 * first failing point, counting the shards' points in shard order; results in front of it are
 * the reference's, results behind it unspecified. */
int interpn_hip_eval_device_sharded(interpn_hip_interp* const* handles, size_t nhandles,
                                    const void* const* const* obs, size_t nobs, void* const* out,
                                    const size_t* npoints, void* const* streams,
                                    uint64_t* first_bad_index);

/* Evaluate on device arrays (asynchronous on `stream`, a hipStream_t; NULL = default stream).
 * `obs` is a HOST array of `nobs` DEVICE pointers, each to `npoints` elements; `out` is a device
 * pointer to `npoints` elements.  Returns as soon as the work is enqueued: one kernel, no copy and
 * no synchronisation, so the call can be captured into a hipGraph.  One exception outside capture:
 * large batches on 4-D multicubic grids whose re-laid table is far beyond the L2 are first
 * counting-sorted by the table position of their footprint (three more launches on `stream`
 * into a scratch block the handle keeps; allocated on the first such call), which makes the
 * 16 table lines a point reads L2 hits instead of misses (option "binned": -1 auto, 0 never,
 * 1 always for N = 2..4).  Results and the first-failing-index contract are unchanged. */
int interpn_hip_eval_device(interpn_hip_interp* h, const void* const* obs, size_t nobs, void* out,
                            size_t npoints, void* stream);

/* ------------------------------------------------------------------------------------------
 * Value and gradient of a MULTILINEAR handle: out[i] = f(x_i) with the bits of interpn_hip_eval_*, and
 * grad[d][i] = df/dx_d at x_i, the derivative of the interpolant with respect to the observation coordinates, from the
 * 2^N corner values the value is made of (one pass over the points, no table traffic beyond a value call's).
 * The reference has no gradient; the definition (DESIGN.md "Gradients") is, per point and at the handle's fma flavour,
 * with the cell origin, the normalised coordinates t[] and the corners V[c] (bit d of c = offset along dimension d) of
 * the value path and lerp(t, y0, y1) the reference's step (dy = y1 - y0; t.mul_add(dy, y0) or y0 + t * dy):
 *   W[c']   = V[c' | 1 << d] - V[c']   for the 2^(N-1) corners c' with bit d clear
 *   s       = W reduced over the dimensions e != d in ascending e with lerp(t[e], lower, upper) (N = 1: s = W[0])
 *   grad[d] = s / h[d]                 h[d] = steps[d], or x1 - x0 of the point's cell on a rectilinear grid
 * every operation rounded in the element type.  It is the slope of the cell the value path selects: outside the grid
 * the edge cell's (the slope of the linear extrapolation), at a knot that of the side the reference's cell rule picks;
 * non-finite inputs propagate.
 *   grad     HOST array of `nobs` pointers, each to `npoints` (`nout`) elements: device pointers in the device form,
 *            host pointers in the host form; grad[d] receives component d.  `out` is required.
 * Checks and statuses are those of interpn_hip_eval_device / _host ("Dimension mismatch"; INTERPN_HIP_ERR_INVALID_ARGUMENT
 * for h, obs, out, grad or one of their entries NULL); a handle of any other method (multicubic, nearest,
 * interpn::one_dim) returns INTERPN_HIP_ERR_UNSUPPORTED before any device work.
 * The device form is ONE kernel for every batch size (no copy, no synchronisation, no allocation: capturable into a
 * graph), reported by interpn_hip_kernel_name: "interpn::k_linear_grad<...>" for N = 2, 3 on the handle's re-laid table,
 * "interpn::k_linear_grad_n<...>" (runtime N on the C-ordered grid) for N = 1, N = 4..8, handles without a table and
 * option force_generic.  INTERPN_HIP_ERR_UNREPRESENTABLE keeps the first-failing-index contract: the host form writes
 * out[0..i) and grad[d][0..i) and leaves the rest untouched; the device form reports i through interpn_hip_finish. */
int interpn_hip_eval_grad_device(interpn_hip_interp* h, const void* const* obs, size_t nobs, void* out,
                                 void* const* grad, size_t npoints, void* stream);
int interpn_hip_eval_grad_host(interpn_hip_interp* h, const void* const* obs, const size_t* obs_lens, size_t nobs,
                               void* out, size_t nout, void* const* grad);

/* ------------------------------------------------------------------------------------------
 * Value and gradient of a MULTICUBIC handle: out[i] = f(x_i) with the bits of interpn_hip_eval_*, and
 * grad[d][i] = df/dx_d at x_i, the derivative of the C1 Hermite interpolant, from the 4^N table values the value is made
 * of (one pass over the points, no table read beyond a value call's).  Entry points of their own: the multilinear pair
 * above keeps returning INTERPN_HIP_ERR_UNSUPPORTED on a multicubic handle.
 * The reference has no gradient; the definition (DESIGN.md "Multicubic gradients") is, per point, at the handle's fma
 * flavour and on the arm of the reference the value path runs (flattened for N <= 4, recursive for N >= 5): per dimension
 * e the value path's footprint origin, saturation class, linearized flag and local coordinate tt[e]; the value tree reduces
 * dimension 0 first and N - 1 last with the 1-D node I_e; the derivative node D_e works on I_e's four inputs from the very
 * c1, c2, c3 (k1) that I_e computes:
 *   Hermite arms     e2 = c2 + c2; e3 = ((1 + 1) + 1) * c3; s = e3.mul_add(tt, e2).mul_add(tt, c1)  (c1 + tt * (e2 + tt * e3))
 *   linearized arms  s = k1        (the value there is k1.mul_add(tt - 1, y1))
 *   component d      levels e < d: the value's partial results; level d: D_d; levels e > d: I_e; one scalar s_d remains
 *   grad[d]          = (Low class along d ? -s_d : s_d) / h[d], one division; h[d] = steps[d], or the spacing the arm's t
 *                    was divided by on a rectilinear grid (h12: None, h01: Low, h23: High)
 * every operation rounded in the element type.  It is the derivative of the polynomial piece the value uses: under
 * linearized extrapolation the held edge slope, without it the extended edge polynomial's; at a knot the piece the
 * reference's cell rule selects; inside the grid continuous across knots along its own axis in exact arithmetic.
 * Non-finite inputs propagate.
 * Arguments, checks, statuses and the first-failing-index contract are those of interpn_hip_eval_grad_device / _host (the
 * shared check is interpn_hip_eval_host's: a wrong number of coordinate arrays on a multicubic handle of at most 4 dimensions
 * is INTERPN_HIP_ERR_REFERENCE_PANIC as there, "Dimension mismatch" otherwise); a handle of any other method returns
 * INTERPN_HIP_ERR_UNSUPPORTED before any device work.
 * The device form is ONE kernel for every batch size (capturable into a graph; the binned, column and sweep paths have no
 * gradient form), reported by interpn_hip_kernel_name: "interpn::k_cubic_grad<...>" for N = 2, 3 on the handle's tiled
 * table, "interpn::k_cubic_grad_n<...>" (runtime N on the C-ordered grid, not tuned) for N = 1, N = 4..8, handles without a
 * table and option force_generic. */
int interpn_hip_eval_cubic_grad_device(interpn_hip_interp* h, const void* const* obs, size_t nobs, void* out,
                                       void* const* grad, size_t npoints, void* stream);
int interpn_hip_eval_cubic_grad_host(interpn_hip_interp* h, const void* const* obs, const size_t* obs_lens, size_t nobs,
                                     void* out, size_t nout, void* const* grad);

/* The same evaluation, telling the caller which path it took.
 *   flags        INTERPN_HIP_EVAL_NO_ALLOC: never allocate (scratch that interpn_hip_reserve has
 *                not provided is then a reason to evaluate in place, reported below).
 *   *path_taken  INTERPN_HIP_PATH_IN_PLACE (one kernel on the points as given),
 *                INTERPN_HIP_PATH_BINNED (points counting-sorted first: 4 launches per slice) or
 *                INTERPN_HIP_PATH_SWEEP (3-D multilinear, large batches: one persistent kernel
 *                whose waves order their points on chip and walk the table in step; 1.25 KiB of
 *                scratch per stream).
 *   *why         for IN_PLACE on a handle that could bin: the reason (INTERPN_HIP_WHY_*); else 0.
 * Either pointer may be NULL.  The sorted path needs scratch (36 B per point of a slice for 4-D
 * f64, slices of at most 2^25 points): one block per stream that uses the handle concurrently, at
 * most 4; streams beyond that take turns through events.  After interpn_hip_reserve(h, n, k) no
 * evaluation of at most n points on at most k streams allocates anything. */
enum { INTERPN_HIP_PATH_IN_PLACE = 0, INTERPN_HIP_PATH_BINNED = 1, INTERPN_HIP_PATH_SWEEP = 2 };
enum { INTERPN_HIP_EVAL_NO_ALLOC = 1 };
enum {
  INTERPN_HIP_WHY_NONE = 0,          /* binned, or binning never applies to this handle */
  INTERPN_HIP_WHY_SMALL_OR_OFF = 1,  /* batch below the break-even size, or option "binned" = 0 */
  INTERPN_HIP_WHY_CAPTURE = 2,       /* `stream` is being captured into a graph */
  INTERPN_HIP_WHY_NO_SCRATCH = 3,    /* no reserved scratch block is free / large enough and allocation was not allowed */
  INTERPN_HIP_WHY_ALLOC_FAILED = 4,  /* the scratch allocation failed */
  INTERPN_HIP_WHY_MISALIGNED = 5     /* sweep evaluation only: `out` or a coordinate array is not 16-byte aligned (its streams are 16-byte accesses) */
};
int interpn_hip_eval_device_ex(interpn_hip_interp* h, const void* const* obs, size_t nobs, void* out,
                               size_t npoints, void* stream, unsigned flags, int* path_taken, int* why);

/* Pre-allocate what device-pointer evaluations of up to `npoints` points on up to `nstreams`
 * concurrent streams need (the sorted path's scratch blocks; nothing for handles that never
 * sort).  Synchronous; may be called again with larger numbers.  It counts every scratch block of
 * the handle that is large enough, whoever made it: behind interpn_hip_reserve_points / _lattice
 * ask for 2 * nstreams, a slice holds one block while its evaluation takes another.  A handle
 * owns at most 4 blocks and `nstreams` is clamped to 4, so both levels can be reserved for two
 * streams at most.  Per-handle counters readable with interpn_hip_get_option: "evals_binned",
 * "evals_in_place", "evals_sweep", "scratch_allocs", "scratch_bytes". */
int interpn_hip_reserve(interpn_hip_interp* h, size_t npoints, int nstreams);

/* Measurement aid (bench.py): with option "stage_timing" = 1 a sorted (binned) single-slice
 * evaluation records HIP events between its launches; this waits for the most recent one and
 * returns its stage durations in milliseconds: ms[0] histogram (+ counter reset), ms[1] scan,
 * ms[2] scatter, ms[3] evaluation kernel.  n >= 4.  INVALID_ARGUMENT when no such evaluation ran. */
int interpn_hip_stage_ms(interpn_hip_interp* h, double* ms, size_t n);

/* Wait for `stream` and report the sticky status of the device evaluations enqueued since the
 * last finish: 0, or INTERPN_HIP_ERR_UNREPRESENTABLE with the smallest failing point index
 * (relative to the evaluation it occurred in) in *first_bad_index.  Clears the sticky word. */
int interpn_hip_finish(interpn_hip_interp* h, void* stream, uint64_t* first_bad_index);

/* Tuning knob: workgroups per CU the launch grid is sized for (default 8). */
int interpn_hip_set_blocks_per_cu(interpn_hip_interp* h, int blocks_per_cu);

/* Per-handle tuning / testing options by name (the list is in the header comment above:
 * "blocks_per_cu", "iters_per_block", "ppl", "axis_regs", "force_generic", "generic_runtime",
 * "generic_vec", "persistent", "axis_lds_kb", "host_chunk", "binned", "deal", "bin_slice_log2" (points
 * per sorted slice, 16..27, default 25: bounds a scratch block), "fma"; read-only: "last_binned" = 1
 * if the most recent device-pointer evaluation sorted its points first, and the counters listed
 * at interpn_hip_reserve).  Their defaults are latched from the
 * INTERPN_HIP_* environment variables when the handle is created.  INTERPN_HIP_ERR_INVALID_ARGUMENT
 * for an unknown name or a value out of range.  Not synchronised against evaluations running
 * concurrently on the same handle. */
int interpn_hip_set_option(interpn_hip_interp* h, const char* name, long long value);
int interpn_hip_get_option(const interpn_hip_interp* h, const char* name, long long* value);

/* Name of the kernel instantiation the most recent evaluation through this handle launched, in
 * rocprofv3's spelling without return type and argument list, e.g.
 * "interpn::k_linear_brick<double, 3, false, true, 1, 2, 2, 0>"; "" before the first launch.
 * (bench.py reports this instead of a hard-coded string.) */
int interpn_hip_kernel_name(const interpn_hip_interp* h, char* buf, size_t buflen);

/* Bytes of the re-laid grid copy the handle keeps (0 = the kernels read the C-ordered `vals`);
 * *step_i / *step_j (optional) receive the layout's brick / tile steps. */
size_t interpn_hip_table_bytes(const interpn_hip_interp* h, int* step_i, int* step_j);

/* Waits only for work enqueued through THIS handle (an event behind its last launch on every
 * caller stream, plus its own staging streams) before its device memory is recycled; other
 * streams of the device keep running.  Launches captured into a graph cannot be tracked: the
 * caller must not replay such a graph after destroying the handle.
 * The handle knows a caller stream by its hipStream_t value (scratch blocks are reused without any
 * command by the stream that used them last, and streams are noted for this wait): synchronise a
 * stream before destroying it while the handle lives, so that a new stream that is given the same
 * value cannot meet work of the old one still in flight. */
void interpn_hip_destroy(interpn_hip_interp* h);

/* ------------------------------------------------------------------------------------------
 * check_bounds (src/multilinear/regular.rs:145-182, rectilinear.rs:109-134; exported to Python
 * as check_bounds_{regular,rectilinear}_{f64,f32}, src/python.rs:87-117, 203-226).
 * out[d] = 1 if any observation violates the bounds of dimension d by atol or more.
 * Host pointers; streamed through the current device.
 * ---------------------------------------------------------------------------------------- */
/* The same check on DEVICE-resident coordinates, limits taken from the handle's grid (the
 * pre-pass of the reference's Python `interpn(..., check_bounds=True)`, src/interpn/__init__.py:
 * 115-132, without moving the points over PCIe).  `obs`: host array of `nobs` device pointers
 * to `npoints` elements of the handle's type; `out`: host, `nout` = ndims bytes.  Synchronous
 * on `stream`. */
int interpn_hip_check_bounds_device(interpn_hip_interp* h, const void* const* obs, size_t nobs,
                                    size_t npoints, double atol, uint8_t* out, size_t nout,
                                    void* stream);

#define INTERPN_HIP_DECLARE_BOUNDS(T, SUFFIX)                                                            \
  int interpn_hip_check_bounds_regular_##SUFFIX(const size_t* dims, size_t ndims, const T* starts,      \
                                                size_t nstarts, const T* steps, size_t nsteps,          \
                                                const T* const* obs, const size_t* obs_lens,            \
                                                size_t nobs, T atol, uint8_t* out, size_t nout);        \
  int interpn_hip_check_bounds_rectilinear_##SUFFIX(const T* const* grids, const size_t* grid_lens,     \
                                                    size_t ngrids, const T* const* obs,                 \
                                                    const size_t* obs_lens, size_t nobs, T atol,        \
                                                    uint8_t* out, size_t nout);

INTERPN_HIP_DECLARE_BOUNDS(double, f64)
INTERPN_HIP_DECLARE_BOUNDS(float, f32)

/* ------------------------------------------------------------------------------------------
 * Field sets — K value grids ("fields") that live on ONE grid, evaluated at the same points: equation-of-state
 * and opacity tables, vector fields, colour channels, scipy's RegularGridInterpolator with trailing value
 * dimensions.  K single handles read the same coordinates K times, search the same cell K times and each visit
 * table lines of their own; a set does the first two once and, on its fused path, fetches lines that hold
 * several fields of one cell.
 *
 * Input     `vals` is field-major: field f is the C-ordered grid at vals + f * field_stride (elements), `nvals`
 *           counts the whole buffer.  `method` as for interpn_hip_create_* (flavour bits included).
 * Checks    all before any device work: nfields == 0, field_stride < prod(dims), nvals < (nfields - 1) *
 *           field_stride + prod(dims): INTERPN_HIP_ERR_INVALID_ARGUMENT; then the single-field creator's checks
 *           on one field, with its statuses, order and strings (a field's length is prod(dims) by construction,
 *           so the reference's "Dimension mismatch" on vals.len() cannot occur; the one on starts / steps can).
 * Contract  row f of a result is bit-identical to what the single handle of field f returns — on both paths,
 *           in both fma flavours — and therefore to the reference.  A point the reference cannot evaluate fails
 *           for every field at once: the host form returns INTERPN_HIP_ERR_UNREPRESENTABLE with out[f][0..i)
 *           written for every f and out[f][i..] untouched; the device form reports i through
 *           interpn_hip_fields_finish.
 * Paths     FUSED (multilinear, N = 2 or 3, regular and rectilinear, f64 and f32, any K): one kernel,
 *           interpn::k_linear_fields, on a table built on the device at creation — one 128-byte line = the 2^N
 *           corners of one cell for P = 128 / (2^N * elem_size) consecutive fields (dimension 0's pair innermost),
 *           the ceil(K / P) lines of a cell contiguous, cells in C order, missing fields zero.  Asynchronous,
 *           allocates nothing, can be captured into a graph.
 *           PER_FIELD (every method, kind, N and type the single handles support, and every set without the
 *           table): K evaluations through K ordinary handles on the caller's stream, each with all the tuned paths
 *           and options of interpn_hip_eval_device_ex (sorting, sweep, in place under capture).
 * Memory    a set owns one device copy of `vals` (or borrows the caller's device buffer, which must outlive it),
 *           K ordinary handles on slices of it (INTERPN_HIP_MEM_DEVICE; each keeps its own copy of a rectilinear
 *           grid's axes, a few KiB), and the fused table: prod(n_d - 1) * ceil(K / P) * 128 bytes
 *           (interpn_hip_fields_layout), built only while it fits a quarter of the free device memory — the rule of
 *           the single handles' tables; otherwise the set is per-field only, which is not an error ("fused_table_bytes"
 *           = 0).  The K handles of a set that has the fused table build their own re-laid tables (up to 16 x a
 *           field each, see the memory note at the top) only when the per-field path is first used outside graph
 *           capture and without INTERPN_HIP_EVAL_NO_ALLOC — a synchronous step of that one call, which reads
 *           INTERPN_HIP_BRICKS then; until then per-field evaluations read the C-ordered fields (same bits).
 * Options   interpn_hip_fields_set_option / _get_option: "fused" = -1 automatic, 0 never, 1 wherever the set has the
 *           table.  Automatic (from measurements): per field where the lines of the table would be
 *           less than 3/4 full (4 K < 3 ceil(K / P) P, e.g. K = 2 in f32), and for 3-D f64 sets whose fields are L2-sized
 *           on batches that the single handles evaluate with the sweep kernel outside graph capture; fused otherwise;
 *           read-only "fused_table_bytes", "nfields", "last_path"; every other name is
 *           passed to the K handles (set: all of them, get: the first), e.g. "blocks_per_cu" (the fused kernel's
 *           persistent grid is sized with it too), "fma", "host_chunk", "sweep".  Latched at creation:
 *           INTERPN_HIP_FIELDS_FUSED=-1|0|1 (0 also skips building the table) and, for tests,
 *           INTERPN_HIP_FIELDS_TABLE_BUDGET=bytes (the table is built only up to this size).
 * Not here  replicate / sharded forms; check_bounds on a set (the bounds are those of the grid: use
 *           interpn_hip_check_bounds_regular_* / _rectilinear_*); interpn::one_dim; a mirror in interpn_hip.hpp
 *           (the reference crate has no such API).
 * Threads   as for single handles; host evaluations of one set are serialised, and they share the sticky status
 *           words with the device form: finish device evaluations before evaluating on host arrays.
 * ---------------------------------------------------------------------------------------- */
typedef struct interpn_hip_fields interpn_hip_fields;

#define INTERPN_HIP_DECLARE_FIELDS(T, SUFFIX)                                                                     \
  int interpn_hip_create_fields_regular_##SUFFIX(int method, const size_t* dims, size_t ndims, const T* starts,  \
                                                 size_t nstarts, const T* steps, size_t nsteps, const T* vals,   \
                                                 size_t nvals, size_t nfields, size_t field_stride,              \
                                                 int vals_mem, int linearize_extrapolation, int device,          \
                                                 interpn_hip_fields** fields);                                   \
  int interpn_hip_create_fields_rectilinear_##SUFFIX(int method, const T* const* grids,                          \
                                                     const size_t* grid_lens, size_t ngrids, const T* vals,      \
                                                     size_t nvals, size_t nfields, size_t field_stride,          \
                                                     int vals_mem, int linearize_extrapolation, int device,      \
                                                     interpn_hip_fields** fields);

INTERPN_HIP_DECLARE_FIELDS(double, f64)
INTERPN_HIP_DECLARE_FIELDS(float, f32)

/* Evaluate every field on device arrays (asynchronous on `stream`): `obs` as for interpn_hip_eval_device, `out` a
 * device pointer, out[f * out_stride + i] = field f at point i (out_stride >= npoints, in elements).  `flags`:
 * INTERPN_HIP_EVAL_NO_ALLOC (the fused path never allocates).  *path_taken (may be NULL): which path ran. */
enum { INTERPN_HIP_FIELDS_PATH_FUSED = 0, INTERPN_HIP_FIELDS_PATH_PER_FIELD = 1 };
int interpn_hip_fields_eval_device(interpn_hip_fields* fields, const void* const* obs, size_t nobs, void* out,
                                   size_t out_stride, size_t npoints, void* stream, unsigned flags, int* path_taken);
/* The same on host arrays (synchronous): chunks of at most 2 Mi points (option "host_chunk"), each chunk's coordinates
 * cross PCIe once for all fields.  nobs == ndims, obs_lens[d] == nout, out_stride >= nout. */
int interpn_hip_fields_eval_host(interpn_hip_fields* fields, const void* const* obs, const size_t* obs_lens, size_t nobs,
                                 void* out, size_t out_stride, size_t nout);
/* interpn_hip_finish for a set: waits for `stream`, reports and clears the sticky status of its device evaluations. */
int interpn_hip_fields_finish(interpn_hip_fields* fields, void* stream, uint64_t* first_bad_index);
/* Waits for the work enqueued through the set (as interpn_hip_destroy does for a handle), then releases everything. */
void interpn_hip_fields_destroy(interpn_hip_fields* fields);
size_t interpn_hip_fields_count(const interpn_hip_fields* fields);
int interpn_hip_fields_ndims(const interpn_hip_fields* fields);
int interpn_hip_fields_elem_size(const interpn_hip_fields* fields);
int interpn_hip_fields_device(const interpn_hip_fields* fields);
/* Kernel of the most recent evaluation: "interpn::k_linear_fields<double, 3, false, true>" (type, N, rectilinear, fma)
 * after a fused one, the first field's kernel after a per-field one. */
int interpn_hip_fields_kernel_name(const interpn_hip_fields* fields, char* buf, size_t buflen);
int interpn_hip_fields_set_option(interpn_hip_fields* fields, const char* name, long long value);
/* "fused", "fused_table_bytes", "nfields", "last_path": the set's own; "evals_binned", "evals_in_place", "evals_sweep":
 * summed over the K handles; every other name: the first handle's (interpn_hip_get_option). */
int interpn_hip_fields_get_option(const interpn_hip_fields* fields, const char* name, long long* value);
/* The fused table of `nfields` fields of `elem_size` (4, 8) bytes on a grid of `dims` (ndims = 2, 3; every axis >= 2):
 * P, ceil(nfields / P) and the table's size.  Needs no device.  INTERPN_HIP_ERR_INVALID_ARGUMENT for anything else. */
int interpn_hip_fields_layout(size_t elem_size, size_t ndims, const size_t* dims, size_t nfields, int* fields_per_line,
                              size_t* lines_per_point, size_t* table_bytes);

/* Gradients of a field set — the K values AND their K x N Jacobian at every point in one call: Newton inversion of an
 * equation-of-state table (K = N), the velocity-gradient tensor of a vector field, `backward` through every channel.
 *
 * Definition  for every field f and point i, out[f * out_stride + i] is what interpn_hip_fields_eval_* returns for field f,
 *           and grad[(f * ndims + d) * grad_stride + i] is component d of what interpn_hip_eval_grad_* returns for the single
 *           handle of field f — for a multicubic set, of interpn_hip_eval_cubic_grad_* ("Value and gradient of a
 *           MULTILINEAR / MULTICUBIC handle" above hold the definitions).  The bits match, in both fma flavours, on both grid
 *           kinds, in f64 and f32.  Both strides are in elements and >= npoints.
 * Paths     FUSED (sets with the fused table: multilinear, N = 2 or 3): one launch of interpn::k_linear_fields_grad on that
 *           table — the cell search, the line-group walk and the table lines of interpn::k_linear_fields; per field N + 1
 *           reduction trees over the pieces a point's 8 lanes hold, K (N + 1) output rows stored as contiguous 64-element
 *           runs.  No scratch, never allocates, can be captured into a graph.
 *           PER_FIELD (multilinear N = 1, 4..8, every multicubic set, sets without the table, "fused" = 0): K calls of
 *           interpn_hip_eval_grad_device (multicubic: interpn_hip_eval_cubic_grad_device) on the K handles with pointers into
 *           the same blocks.
 *           Reported with INTERPN_HIP_FIELDS_PATH_* through *path_taken and the option "last_path";
 *           interpn_hip_fields_kernel_name says "interpn::k_linear_fields_grad<double, 3, false, true>" after a fused call.
 * Options   "fused" (-1, 0, 1) means what it means for values.  Automatic: fused wherever the set has the table (both
 *           paths are one-pass kernels, so the value rule's sweep clause does not apply; DESIGN.md "Field-set gradients").
 * Checks    those of interpn_hip_fields_eval_device / _host in their order, a nearest set: INTERPN_HIP_ERR_UNSUPPORTED
 *           (before the observation-point checks and any device work); npoints == 0: INTERPN_HIP_OK whatever the pointers
 *           are; then out or grad NULL, out_stride or grad_stride < npoints, an obs[d] NULL: INTERPN_HIP_ERR_INVALID_ARGUMENT.
 * Failing   a point the reference cannot evaluate fails for every field at once.  Device form: interpn_hip_fields_finish
 * points    reports its index.  Host form: INTERPN_HIP_ERR_UNREPRESENTABLE with out[f][0..i) and grad[f][d][0..i) written
 *           for every f, d and everything behind untouched. */
/* Asynchronous on `stream`; `obs`, `out`, `grad`: device.  `flags`: INTERPN_HIP_EVAL_NO_ALLOC.  *path_taken (may be NULL). */
int interpn_hip_fields_eval_grad_device(interpn_hip_fields* fields, const void* const* obs, size_t nobs, void* out,
                                        size_t out_stride, void* grad, size_t grad_stride, size_t npoints, void* stream,
                                        unsigned flags, int* path_taken);
/* The same on host arrays (synchronous): chunks of at most 2 Mi points (option "host_chunk"), each chunk's coordinates cross
 * PCIe once for all fields, the K (N + 1) result rows are copied back row by row.  nobs == ndims, obs_lens[d] == nout. */
int interpn_hip_fields_eval_grad_host(interpn_hip_fields* fields, const void* const* obs, const size_t* obs_lens, size_t nobs,
                                      void* out, size_t out_stride, void* grad, size_t grad_stride, size_t nout);

/* Point-major field sets — the points as ONE array of shape (npoints, N), the results as ONE array of shape (npoints, K):
 * positions or ray samples in, a velocity or an RGBA per point out, without a transpose on either side.
 *
 * Definition  coordinate d of point i is pts[i * point_stride + d] (point_stride >= ndims, in ELEMENTS; elements d >= ndims
 *           of a row are never read, the last row's may not exist); field f of point i goes to out[i * out_stride + f]
 *           (out_stride >= nfields; elements f >= nfields of a row are never written).  `pts` and `out` must not overlap.
 *           Every result has the bits of interpn_hip_fields_eval_device on the de-interleaved columns.
 * Paths     FUSED (sets with the fused table: multilinear N = 2, 3): one launch of interpn::k_linear_fields_points on
 *           that table — k_linear_fields' statements between a row load (dense rows: the wave's span through LDS; any other
 *           stride: element loads) and a row store (the wave's results staged as a [64][8] tile in LDS and stored as
 *           contiguous runs: one run of 64 K elements per wave where out_stride == K <= 8).  No scratch, never allocates,
 *           can be captured into a graph.
 *           SPLIT (everything else: cubic, nearest, N = 1, N >= 4, sets without the table, "fused" = 0): per slice
 *           interpn::k_split_points de-interleaves the rows into scratch, the column form evaluates them into K scratch
 *           rows (fused or per field by the option "fused" and its rule), interpn::k_join_fields writes the caller's rows.
 *           One scratch block, from the first field's handle, holds a slice: (N + K) arrays within 64 MiB together, 256
 *           points at least.  Under graph capture or with INTERPN_HIP_EVAL_NO_ALLOC only reserved blocks are used
 *           (INTERPN_HIP_ERR_OUT_OF_MEMORY without one); interpn_hip_fields_reserve_points provides them.
 * Options   "points_path" = -1 automatic (fused wherever the set has the table and "fused" is not 0),
 *           1 fused or INTERPN_HIP_ERR_UNSUPPORTED, 2 split.  Read-only "last_points_path" (INTERPN_HIP_FIELDS_POINTS_PATH_*;
 *           -1 before any).  "points_slice" (testing): points per slice of the split path.  interpn_hip_fields_kernel_name
 *           reports "interpn::k_linear_fields_points<double, 3, false, true>" after a fused call.
 * Checks    before any device work, in this order: fields NULL; point_stride < ndims, out_stride < nfields:
 *           INTERPN_HIP_ERR_INVALID_ARGUMENT; npoints == 0: INTERPN_HIP_OK whatever the pointers are; pts or out NULL, or a
 *           block whose bytes do not fit size_t: INTERPN_HIP_ERR_INVALID_ARGUMENT; "points_path" = 1 without the table:
 *           INTERPN_HIP_ERR_UNSUPPORTED.
 * Failing   device form: interpn_hip_fields_finish reports the first failing point of the whole call, on every path.  Host
 * points    form: the set's status; exactly rows [0, i) are written, their first K elements only, everything else is left
 *           as it was. */
enum { INTERPN_HIP_FIELDS_POINTS_PATH_FUSED = 0, INTERPN_HIP_FIELDS_POINTS_PATH_SPLIT = 1 };
/* Asynchronous on `stream`; `pts`, `out`: device.  `flags`: INTERPN_HIP_EVAL_NO_ALLOC.  *path_taken (may be NULL). */
int interpn_hip_fields_eval_points_device(interpn_hip_fields* fields, const void* pts, size_t point_stride, size_t npoints,
                                          void* out, size_t out_stride, void* stream, unsigned flags, int* path_taken);
/* The same on host arrays, synchronous: chunks of 2 Mi points (option "host_chunk"), a chunk's rows uploaded with one copy,
 * only the first K elements of the rows in front of a failing point downloaded. */
int interpn_hip_fields_eval_points_host(interpn_hip_fields* fields, const void* pts, size_t point_stride, size_t npoints,
                                        void* out, size_t out_stride);
/* Scratch blocks for split-path evaluations of up to `npoints` points on up to `nstreams` concurrent streams (blocks of
 * the first field's handle; per-field evaluations of large batches may want interpn_hip_reserve on the handles' paths as
 * well, which a set does not expose: under NO_ALLOC they evaluate in place). */
int interpn_hip_fields_reserve_points(interpn_hip_fields* fields, size_t npoints, int nstreams);

/* Point-major gradients of a field set — the points as ONE (npoints, N) array, the K values as ONE (npoints, K) array and
 * their Jacobian as ONE (npoints, K, N) array: particle positions or a model's (..., N) tensor in, a feature vector and its
 * derivative with respect to the position out, without a transpose on either side.
 *
 * Definition  coordinate d of point i is pts[i * point_stride + d], as for interpn_hip_fields_eval_points_* (elements
 *           d >= ndims of a row are never read).  out[i * out_stride + f] has the bits of interpn_hip_fields_eval_points_*
 *           (those of interpn_hip_fields_eval_* on the columns); jac[i * jac_stride + f * ndims + d] has the bits of
 *           grad[(f * ndims + d) * grad_stride + i] of interpn_hip_fields_eval_grad_* on the columns, in both fma flavours.
 *           Strides in ELEMENTS, out_stride >= nfields, jac_stride >= nfields * ndims; elements of a row beyond its first
 *           K (values) or K * ndims (Jacobian) are never written.  The three blocks must not overlap.
 * Paths     FUSED (sets with the fused table: multilinear N = 2, 3): one launch of interpn::k_linear_fields_points_grad on
 *           that table — the row load of k_linear_fields_points, the cell search, piece fetch and N + 1 trees per field of
 *           k_linear_fields_grad, and per line group a point-major LDS tile from which a point's min(P, K - f0) values and
 *           min(P, K - f0) * N components are stored lane-contiguously (jac_stride == K * N and one line group: one run of
 *           64 K N elements per wave).  The cell widths travel through LDS beside t[N] and the storing lane does the one
 *           division of a component.  No scratch, never allocates, can be captured into a graph.
 *           SPLIT (every multicubic set, multilinear N = 1 and 4..8, sets without the table, "fused" = 0, "points_path" =
 *           2): per slice interpn::k_split_points de-interleaves the rows into scratch, interpn_hip_fields_eval_grad_device
 *           evaluates them into K + K N scratch rows (fused or per field by its own rule), interpn::k_join_fields writes
 *           the value rows and, with K N "fields", the Jacobian rows.  One scratch block, from the first field's handle,
 *           holds a slice: N + K (N + 1) arrays within 64 MiB together, 256 points at least.  Under graph capture or with
 *           INTERPN_HIP_EVAL_NO_ALLOC only reserved blocks are used (INTERPN_HIP_ERR_OUT_OF_MEMORY without one);
 *           interpn_hip_fields_reserve_points_grad provides them.
 *           Reported with INTERPN_HIP_FIELDS_POINTS_PATH_* through *path_taken and the option "last_points_path";
 *           interpn_hip_fields_kernel_name says "interpn::k_linear_fields_points_grad<double, 3, false, true>" after a
 *           fused call.
 * Options   "points_path" (-1, 1, 2) and "points_slice" mean what they mean for interpn_hip_fields_eval_points_*; "fused"
 *           what it means for interpn_hip_fields_eval_grad_*.  Automatic: fused wherever the set has the table and "fused"
 *           is not 0, except sets of two fields per table line and four line groups or more (3-D f64, K >= 7), where the
 *           fused kernel measured level with the split path at best.
 * Checks    before any device work, in this order: fields NULL: INTERPN_HIP_ERR_INVALID_ARGUMENT; a nearest set:
 *           INTERPN_HIP_ERR_UNSUPPORTED; point_stride < ndims, out_stride < nfields, jac_stride < nfields * ndims:
 *           INTERPN_HIP_ERR_INVALID_ARGUMENT; npoints == 0: INTERPN_HIP_OK whatever the pointers are; pts, out or jac NULL,
 *           or a block whose bytes do not fit size_t: INTERPN_HIP_ERR_INVALID_ARGUMENT; unknown flags:
 *           INTERPN_HIP_ERR_INVALID_ARGUMENT; "points_path" = 1 without the table: INTERPN_HIP_ERR_UNSUPPORTED.
 * Failing   device form: interpn_hip_fields_finish reports the first failing point of the whole call, on every path.  Host
 * points    form: the set's status; exactly rows [0, i) of both blocks are written, their first K and K * ndims elements
 *           only, everything else is left as it was. */
/* Asynchronous on `stream`; `pts`, `out`, `jac`: device.  `flags`: INTERPN_HIP_EVAL_NO_ALLOC.  *path_taken (may be NULL). */
int interpn_hip_fields_eval_points_grad_device(interpn_hip_fields* fields, const void* pts, size_t point_stride, size_t npoints,
                                               void* out, size_t out_stride, void* jac, size_t jac_stride, void* stream,
                                               unsigned flags, int* path_taken);
/* The same on host arrays, synchronous: chunks of 2 Mi points (option "host_chunk"), a chunk's rows uploaded with one copy,
 * only the first K and K * ndims elements of the rows in front of a failing point downloaded. */
int interpn_hip_fields_eval_points_grad_host(interpn_hip_fields* fields, const void* pts, size_t point_stride, size_t npoints,
                                             void* out, size_t out_stride, void* jac, size_t jac_stride);
/* Scratch blocks for split-path evaluations of up to `npoints` points on up to `nstreams` concurrent streams (blocks of
 * the first field's handle). */
int interpn_hip_fields_reserve_points_grad(interpn_hip_fields* fields, size_t npoints, int nstreams);

/* ------------------------------------------------------------------------------------------
 * Lattice evaluation — the points are the tensor product of N coordinate vectors, one per axis: re-gridding,
 * RegularGridInterpolator on a meshgrid, resampling a volume, refining a table.  The caller passes the N vectors
 * (sum of their lengths coordinates) instead of N arrays of prod(lengths) coordinates; out[i_0, .., i_{N-1}] (C order,
 * last axis contiguous) is the interpolant at (axes[0][i_0], .., axes[N-1][i_{N-1}]).  The vectors need not be sorted.
 *
 * Contract  every result is bit-identical to what interpn_hip_eval_device gives for the expanded point, in both fma
 *           flavours, and therefore to the reference.
 * Paths     FUSED (multilinear and multicubic, N = 2 or 3, regular and rectilinear, f64 and f32, grids that 32 bits
 *           index): interpn::k_lattice_axes turns every axis coordinate into a record (cell, normalized coordinate,
 *           cubic class, rectilinear spacing ratios) with the device functions of the per-point kernels;
 *           interpn::k_lattice_rows then reduces dims 0..N-2 once per output row and grid column of the last axis into
 *           an LDS line and evaluates every output of the row as one node of the last dimension.  Per point it moves
 *           sizeof(T) bytes instead of (N + 1) sizeof(T).  Condition: four lines of n_{N-1} elements fit the LDS budget
 *           of rectilinear axis images (20 KiB; option "axis_lds_kb").
 *           EXPANDED (everything else: nearest, N = 1, N >= 4, longer last axes): interpn::k_lattice_expand writes the
 *           coordinates of a slice of the lattice (64 MiB at most) into scratch, and the slice goes through
 *           interpn_hip_eval_device_ex with all its paths and options.
 * Options   "lattice" = -1 automatic, 0 never fused, 1 fused wherever covered.  Automatic takes the fused path when,
 *           in addition, the lattice has a row for every wave of the device (prod(m_0..m_{N-2}) >= 4 x CUs) and the last
 *           grid axis is not much longer than the last lattice axis (n_{N-1} <= 4 max(m_{N-1}, 64)): DESIGN.md.
 *           Read-only "last_lattice_path" (INTERPN_HIP_LATTICE_PATH_*; -1 before any).  interpn_hip_kernel_name reports
 *           "interpn::k_lattice_rows<T, method, N, rectilinear, fma>" after a fused evaluation.
 * Scratch   both paths work in one of the handle's scratch blocks (records: 16 to 64 bytes per axis coordinate; the
 *           expanded slice), under the rules of interpn_hip_eval_device_ex: one block per concurrent stream, at most 4,
 *           allocated on first use unless INTERPN_HIP_EVAL_NO_ALLOC is given; interpn_hip_reserve_lattice provides
 *           them in advance.  Without a block the call returns INTERPN_HIP_ERR_OUT_OF_MEMORY.  A stream under graph
 *           capture never allocates and touches no event of a block: reserve or evaluate once before capturing, and keep
 *           other streams away from the handle while the graph replays.
 * Checks    h, axes, axis_lens, out or an axes[d] NULL: INTERPN_HIP_ERR_INVALID_ARGUMENT; interpn::one_dim handles:
 *           INTERPN_HIP_ERR_UNSUPPORTED; naxes != ndims: what interpn_hip_eval_device returns for the wrong number of
 *           coordinate arrays; a point count beyond size_t: INTERPN_HIP_ERR_INVALID_ARGUMENT; more than 2^31 axis
 *           coordinates in all: INTERPN_HIP_ERR_UNSUPPORTED; any axis_lens[d] == 0: no points, INTERPN_HIP_OK, nothing
 *           written.
 * Failing   regular grids only (rectilinear grids never fail a point and propagate NaN): a coordinate the reference
 * points    cannot convert (NaN, +-inf, |floc| >= 2^63) at position j of axis d fails every lattice point that uses it.
 *           interpn_hip_finish reports the reference loop's first failure in C order,
 *           min over bad (d, j) of j * prod(axis_lens[e], e > d), with the handle's status for such points.
 * ---------------------------------------------------------------------------------------- */
enum { INTERPN_HIP_LATTICE_PATH_FUSED = 0, INTERPN_HIP_LATTICE_PATH_EXPANDED = 1 };
/* Asynchronous on `stream`.  `axes`: HOST array of `naxes` DEVICE pointers, axes[d] to axis_lens[d] coordinates; `out`: device,
 * prod(axis_lens) elements.  `flags`: INTERPN_HIP_EVAL_NO_ALLOC.  *path_taken (may be NULL): INTERPN_HIP_LATTICE_PATH_*. */
int interpn_hip_eval_lattice_device(interpn_hip_interp* h, const void* const* axes, const size_t* axis_lens, size_t naxes,
                                    void* out, void* stream, unsigned flags, int* path_taken);
/* The same on host arrays, synchronous (chunks of leading-axis indices, 2^25 points each).  On a failing point the status
 * is the handle's ("Unrepresentable coordinate value"), exactly out[0..first_bad) is written, the rest of `out` is left
 * as it was, and *first_bad_index (may be NULL) receives the index.  Shares the sticky status word with the device form:
 * finish device evaluations first. */
int interpn_hip_eval_lattice_host(interpn_hip_interp* h, const void* const* axes, const size_t* axis_lens, size_t naxes,
                                  void* out, uint64_t* first_bad_index);
/* Scratch blocks for lattices of up to these axis lengths on up to `nstreams` concurrent streams, whichever path the
 * options choose at evaluation time.  Synchronous.  An expanded slice that the handle would sort or sweep takes a
 * second block while it holds the first; without one it is evaluated in place.  interpn_hip_reserve counts every block
 * that is large enough, these among them: call it with 2 * nstreams behind this call (see interpn_hip_reserve_points). */
int interpn_hip_reserve_lattice(interpn_hip_interp* h, const size_t* axis_lens, size_t naxes, int nstreams);
/* Which path a lattice of `axis_lens` on a grid of `dims` takes in automatic mode on an MI355X, the fused workgroup's
 * LDS bytes (0 when expanded) and the overflow-checked point count.  Needs no device; honours the INTERPN_HIP_*
 * variables a new handle would latch (AXIS_LDS_KB, LATTICE, FORCE_GENERIC).  `method`: INTERPN_HIP_LINEAR / _CUBIC /
 * _NEAREST.  INTERPN_HIP_ERR_INVALID_ARGUMENT: element size, method, ndims outside 1..8, an axis below the method's
 * minimum, a point count beyond size_t. */
int interpn_hip_lattice_plan(size_t elem_size, int method, size_t ndims, const size_t* dims, const size_t* axis_lens,
                             int* path, size_t* lds_bytes, size_t* npoints);

/* ------------------------------------------------------------------------------------------
 * Gradients on a lattice — the value and d/dx of every lattice point in one pass: forces from a potential table on a
 * finer mesh, shading normals of a resampled volume, the partial derivatives of a refined equation-of-state table.
 * `axes`, `axis_lens`, `naxes` as for interpn_hip_eval_lattice_device; `grad`: HOST array of `naxes` pointers to
 * prod(axis_lens) elements each, as in interpn_hip_eval_grad_device; grad[d][p] is the derivative with respect to
 * coordinate d at the lattice point p (C order).
 *
 * Contract  nothing new is defined: out[p] has the bits of interpn_hip_eval_lattice_device, and grad[d][p] the bits of
 *           component d of interpn_hip_eval_grad_device (multilinear handles) or interpn_hip_eval_cubic_grad_device
 *           (multicubic handles) on the expanded point, in both fma flavours.  Nearest and interpn::one_dim handles:
 *           INTERPN_HIP_ERR_UNSUPPORTED before any device work, as for those entry points.
 * Paths     FUSED (the coverage of interpn_hip_eval_lattice_device's fused path): the unchanged interpn::k_lattice_axes
 *           launch, then interpn::k_lattice_grad_rows, in which a wave owns L lines instead of one — multilinear L =
 *           N + 1 (the value, one per component d < N-1, and the differences along the last axis, which the definition
 *           takes before it reduces), multicubic L = N (the value and one per component d < N-1; the last component is
 *           the derivative node of the value line).  A wave's lines lie packed: the condition is
 *           4 * round16(L * n_{N-1} * sizeof(T)) within the budget "axis_lds_kb".  Per point it moves (N + 1) sizeof(T)
 *           bytes instead of (2 N + 1) sizeof(T).
 *           EXPANDED (everything else): the expanded path of interpn_hip_eval_lattice_device, each slice through
 *           interpn_hip_eval_grad_device / interpn_hip_eval_cubic_grad_device.
 * Options   "lattice" governs value and gradient calls alike; automatic mode applies the value path's two rules (carried
 *           over; the measured rows ask for no tighter ones: DESIGN.md section 18).  "last_lattice_path" and *path_taken as for the
 *           value; interpn_hip_kernel_name reports "interpn::k_lattice_grad_rows<T, method, N, rectilinear, fma>" after a
 *           fused call.
 * Scratch   exactly the value call's (records when fused; flags and one coordinate slice when expanded), under the same
 *           rules, graph capture included.  interpn_hip_reserve_lattice serves gradient calls: there is no separate
 *           reserve entry point.
 * Checks    those of interpn_hip_eval_lattice_device in their order; then a handle that is neither multilinear nor
 *           multicubic: INTERPN_HIP_ERR_UNSUPPORTED; then `grad` or a grad[d] NULL: INTERPN_HIP_ERR_INVALID_ARGUMENT.  An
 *           empty axis: INTERPN_HIP_OK, nothing written.
 * Failing   as for the value call: the same first index in C order through interpn_hip_finish.
 * points
 * ---------------------------------------------------------------------------------------- */
int interpn_hip_eval_lattice_grad_device(interpn_hip_interp* h, const void* const* axes, const size_t* axis_lens, size_t naxes,
                                         void* out, void* const* grad, void* stream, unsigned flags, int* path_taken);
/* The same on host arrays, synchronous (chunks of leading-axis indices, about 2^25 / (N + 1) points each; option
 * "host_chunk": points).  On a failing point the status is the handle's, exactly out[0..first_bad) and
 * grad[d][0..first_bad) are written, the rest is left as it was, and *first_bad_index (may be NULL) receives the index. */
int interpn_hip_eval_lattice_grad_host(interpn_hip_interp* h, const void* const* axes, const size_t* axis_lens, size_t naxes,
                                       void* out, void* const* grad, uint64_t* first_bad_index);
/* interpn_hip_lattice_plan for a value-and-gradient call (no device; the same environment latches and statuses), except
 * that the nearest method has no gradient: INTERPN_HIP_ERR_UNSUPPORTED. */
int interpn_hip_lattice_grad_plan(size_t elem_size, int method, size_t ndims, const size_t* dims, const size_t* axis_lens,
                                  int* path, size_t* lds_bytes, size_t* npoints);

/* ------------------------------------------------------------------------------------------
 * Field sets on a lattice — K fields of one grid re-gridded onto the tensor product of N coordinate vectors in one pass:
 * resizing an (H, W, C) image or a (D, H, W, C) volume, re-gridding several variables of a simulation onto a finer mesh,
 * refining a table of K quantities.  `axes`, `axis_lens`, `naxes` as for interpn_hip_eval_lattice_device.
 *
 * Layouts   INTERPN_HIP_FIELDS_LATTICE_FIELD_MAJOR: out[f * out_stride + p], out_stride >= prod(axis_lens) — shape (K, *m);
 *           INTERPN_HIP_FIELDS_LATTICE_FIELDS_LAST: out[p * out_stride + f], out_stride >= K — shape (*m, K), the
 *           channel-last layout; p is the lattice index in C order, strides in ELEMENTS.  Nothing is written at f >= K,
 *           behind a row's first K elements, or between two fields' blocks.  `out` must not overlap the axes.
 * Contract  field f of every result has the bits of interpn_hip_eval_lattice_device on the handle of field f alone, on
 *           both paths, in both fma flavours, and therefore the reference's.
 * Paths     FUSED (multilinear and multicubic, N = 2 or 3, regular and rectilinear, f64 and f32, grids that 32 bits index):
 *           ONE launch of interpn::k_lattice_axes for all K fields (the records do not depend on the field), then ONE launch
 *           of interpn::k_lattice_fields_rows on the set's field-major `vals` — no re-laid table, so it is the one-pass
 *           multicubic form of a set as well.  A wave owns a row and processes the fields in groups of G: G LDS lines (dims
 *           0..N-2 of each field reduced at every grid column of the last axis), then per output the last axis's record once
 *           and one node per field.  Fields-last results leave through a [64][G] LDS tile as contiguous runs (one run of
 *           64 K elements per wave and chunk where out_stride == K == G).  G = the largest g <= min(K, 8) with
 *           4 * (g * line + tile(g)) within the LDS budget of interpn_hip_eval_lattice_device ("axis_lds_kb"), line =
 *           n_{N-1} elements rounded up to 16 bytes, tile(g) = 64 * (g | 1) elements rounded up to 16 bytes for
 *           fields-last and 0 for field-major results; K > G: ceil(K / G) passes per row.  Takes a records block of the
 *           FIRST field's handle under the rules of interpn_hip_eval_lattice_device; capturable after
 *           interpn_hip_fields_reserve_lattice; builds none of the handles' deferred tables.
 *           PER_FIELD (everything else: nearest, N = 1, N >= 4, last axes whose line does not fit, "lattice" = 0, grids 32
 *           bits do not index, "force_generic"): K calls of interpn_hip_eval_lattice_device's path through the K handles.
 *           Field-major results go straight into the caller's rows; fields-last results go, per slice of whole leading-axis
 *           indices (K rows within 64 MiB together, one index at least; option "points_slice" = points, for tests), into
 *           scratch rows of the first handle and through interpn::k_join_fields.
 * Options   "lattice" and "axis_lds_kb" (forwarded to the K handles; the fused path reads the first one's).  "lattice" = 1:
 *           fused wherever covered and G >= 1; -1 automatic: the rules of interpn_hip_eval_lattice_device and G >= 1
 *           (measured, DESIGN.md section 16: no further rule for short runs per point).  Read-only "last_lattice_path"
 *           (INTERPN_HIP_FIELDS_LATTICE_PATH_*; -1 before any) and "last_lattice_group" (G of the last fused evaluation).
 *           interpn_hip_fields_kernel_name reports "interpn::k_lattice_fields_rows<T, method, N, rectilinear, fma,
 *           fields_last>" after a fused evaluation.
 * Checks    before any device work, in this order: fields NULL: INTERPN_HIP_ERR_INVALID_ARGUMENT; the checks of
 *           interpn_hip_eval_lattice_device in their order with their statuses (an empty axis: INTERPN_HIP_OK, nothing
 *           written); then a layout value other than the two, out_stride below prod(axis_lens) (field-major) or below K
 *           (fields-last), or a result whose bytes do not fit size_t: INTERPN_HIP_ERR_INVALID_ARGUMENT.
 * Failing   regular grids only.  The first failing lattice index in C order over axis_lens is the same for every field
 * points    (the field axis is not part of it).  Device form: interpn_hip_fields_finish reports it, on both paths.  Host
 *           form: the set's status, *first_bad_index = i, and exactly the results in front of it are written: out[f][0..i)
 *           for every f (field-major), rows [0, i) (fields-last); everything else is left as it was.
 * ---------------------------------------------------------------------------------------- */
enum { INTERPN_HIP_FIELDS_LATTICE_FIELD_MAJOR = 0, INTERPN_HIP_FIELDS_LATTICE_FIELDS_LAST = 1 };
enum { INTERPN_HIP_FIELDS_LATTICE_PATH_FUSED = 0, INTERPN_HIP_FIELDS_LATTICE_PATH_PER_FIELD = 1 };
/* Asynchronous on `stream`.  `axes`: HOST array of `naxes` DEVICE pointers; `out`: device.  `flags`:
 * INTERPN_HIP_EVAL_NO_ALLOC.  *path_taken (may be NULL): INTERPN_HIP_FIELDS_LATTICE_PATH_*. */
int interpn_hip_fields_eval_lattice_device(interpn_hip_fields* fields, const void* const* axes, const size_t* axis_lens,
                                           size_t naxes, void* out, size_t out_stride, int layout, void* stream, unsigned flags,
                                           int* path_taken);
/* The same on host arrays, synchronous: chunks of leading-axis indices of about 2^25 / K points each (option "host_chunk":
 * points per chunk).  Shares the sticky status words with the device form: finish device evaluations first. */
int interpn_hip_fields_eval_lattice_host(interpn_hip_fields* fields, const void* const* axes, const size_t* axis_lens,
                                         size_t naxes, void* out, size_t out_stride, int layout, uint64_t* first_bad_index);
/* Scratch blocks for lattices of up to these axis lengths on up to `nstreams` concurrent streams: every handle gets what
 * interpn_hip_reserve_lattice gives it, the first handle twice the blocks, each also large enough for the per-field
 * path's slice of K rows.  A handle holds 4 blocks at most, and a per-field evaluation with fields-last results holds two
 * of the first handle's at a time: for THAT form the guarantee covers two concurrent streams, not more — a third stream's
 * evaluation under INTERPN_HIP_EVAL_NO_ALLOC or graph capture can return INTERPN_HIP_ERR_OUT_OF_MEMORY.  The fused path
 * and field-major results are covered up to 4 streams.  Synchronous. */
int interpn_hip_fields_reserve_lattice(interpn_hip_fields* fields, const size_t* axis_lens, size_t naxes, int nstreams);
/* Which path (INTERPN_HIP_FIELDS_LATTICE_PATH_*) a set of `nfields` fields takes on a lattice of `axis_lens` on a grid of
 * `dims` with results in `layout`, G and the fused workgroup's LDS bytes (both 0 on the per-field path) and the
 * overflow-checked point count.  Needs no device; arguments, statuses and latched environment as for
 * interpn_hip_lattice_plan, checked first; then nfields == 0 or another layout value: INTERPN_HIP_ERR_INVALID_ARGUMENT. */
int interpn_hip_fields_lattice_plan(size_t elem_size, int method, size_t ndims, const size_t* dims, const size_t* axis_lens,
                                    size_t nfields, int layout, int* path, size_t* group, size_t* lds_bytes, size_t* npoints);

/* ------------------------------------------------------------------------------------------
 * Field-set gradients on a lattice — the values of K fields AND their K x N Jacobian on the tensor product of N coordinate
 * vectors in one pass: the Jacobian (and its determinant) of a displacement field resampled onto a finer mesh, the
 * velocity-gradient tensor of a re-gridded vector field, the per-channel gradients of a resized (H, W, C) image, the partial
 * derivatives of all K quantities of a refined table.  `axes`, `axis_lens`, `naxes` as for interpn_hip_eval_lattice_device.
 *
 * Layouts   the two of "Field sets on a lattice", strides in ELEMENTS, p the lattice index in C order, d the coordinate:
 *           INTERPN_HIP_FIELDS_LATTICE_FIELD_MAJOR: out[f * out_stride + p], shape (K, *m), and
 *           jac[(f * N + d) * jac_stride + p], shape (K, N, *m); both strides >= prod(axis_lens) — the convention of
 *           interpn_hip_fields_eval_grad_device.
 *           INTERPN_HIP_FIELDS_LATTICE_FIELDS_LAST: out[p * out_stride + f], shape (*m, K), out_stride >= K, and
 *           jac[p * jac_stride + f * N + d], shape (*m, K, N), jac_stride >= K * N — the convention of
 *           interpn_hip_fields_eval_points_grad_device.
 *           Nothing is written outside those elements: padding columns of a wider row stay as they were.  `out`, `jac`
 *           and the axes must not overlap.
 * Contract  nothing new is defined: out for (f, p) has the bits of interpn_hip_fields_eval_lattice_device (and so of
 *           interpn_hip_eval_lattice_device on the handle of field f alone), and jac for (f, d, p) the bits of grad[d][p] of
 *           interpn_hip_eval_lattice_grad_device on the handle of field f alone, on both paths, in both fma flavours, in
 *           f64 and f32, on regular and rectilinear grids.
 * Paths     FUSED (multilinear and multicubic, N = 2 or 3, grids that 32 bits index): ONE launch of interpn::k_lattice_axes
 *           on the first field's description, then ONE launch of interpn::k_lattice_fields_grad_rows — the field loop,
 *           groups and tile of interpn::k_lattice_fields_rows around the L lines per field of interpn::k_lattice_grad_rows
 *           (multilinear L = N + 1, multicubic L = N).  A wave owns a row and G x L packed lines; per chunk of 64 outputs a
 *           lane loads the last axis's record, width and sign once and computes, per field of the group, the value and the
 *           N components (one IEEE division each).  Field-major results leave as N + 1 coalesced stores per field;
 *           fields-last results through a [64] x P LDS tile, P = (G (N + 1)) | 1, as contiguous runs (where jac_stride ==
 *           K N == G N: one run of 64 K N elements per wave and chunk).  G = the largest g <= min(K, 8) with
 *           4 * (round16(g * L * n_{N-1} * sizeof(T)) + tile(g)) within the LDS budget "axis_lds_kb", tile(g) =
 *           round16(64 * ((g (N + 1)) | 1) * sizeof(T)) for fields-last and 0 for field-major results; K > G: ceil(K / G)
 *           passes per row.  At the default 20 KiB a fields-last f64 3-D call never has G > 2 (and G = 2 only for last grid
 *           axes of at most 8 or 10 entries): the tile takes the room, and "axis_lds_kb" is the knob.  Takes a records
 *           block of the FIRST field's handle under the rules of interpn_hip_eval_lattice_device; capturable after
 *           interpn_hip_fields_reserve_lattice_grad; builds none of the handles' deferred tables.
 *           PER_FIELD (everything else: N = 1, N >= 4, a line beyond the budget, "lattice" = 0, "force_generic", grids 32
 *           bits do not index): K calls of interpn_hip_eval_lattice_grad_device's path through the K handles.  Field-major
 *           results go straight into the caller's rows (grad[d] = jac + (f * N + d) * jac_stride); fields-last results
 *           go, per slice of whole leading-axis indices (K (N + 1) rows within 64 MiB together, one index at least;
 *           option "points_slice" = points, for tests), into scratch rows of the first handle and through two launches of
 *           interpn::k_join_fields, K rows into `out` and K N rows into `jac`.
 * Options   "lattice" and "axis_lds_kb" as for the value form; automatic mode applies the rules of
 *           interpn_hip_eval_lattice_grad_device and G >= 1, no rule of its own.  "last_lattice_path"
 *           and "last_lattice_group" are updated; interpn_hip_fields_kernel_name reports
 *           "interpn::k_lattice_fields_grad_rows<T, method, N, rectilinear, fma, fields_last>" after a fused evaluation.
 * Checks    before any device work, in this order: fields NULL: INTERPN_HIP_ERR_INVALID_ARGUMENT; the checks of
 *           interpn_hip_fields_eval_lattice_device on the lattice in their order (an empty axis: INTERPN_HIP_OK, nothing
 *           written); a nearest set: INTERPN_HIP_ERR_UNSUPPORTED; then `jac` NULL, a layout value other than the two, a
 *           stride below its minimum, or a result whose bytes do not fit size_t: INTERPN_HIP_ERR_INVALID_ARGUMENT.
 * Failing   as for "Field sets on a lattice": one first failing index in C order for every field, through
 * points    interpn_hip_fields_finish on both paths (the fused path uses the first handle's word).
 * ---------------------------------------------------------------------------------------- */
/* Asynchronous on `stream`.  `axes`: HOST array of `naxes` DEVICE pointers; `out`, `jac`: device.  `flags`:
 * INTERPN_HIP_EVAL_NO_ALLOC.  *path_taken (may be NULL): INTERPN_HIP_FIELDS_LATTICE_PATH_*. */
int interpn_hip_fields_eval_lattice_grad_device(interpn_hip_fields* fields, const void* const* axes, const size_t* axis_lens,
                                                size_t naxes, void* out, size_t out_stride, void* jac, size_t jac_stride,
                                                int layout, void* stream, unsigned flags, int* path_taken);
/* The same on host arrays, synchronous: chunks of leading-axis indices of about 2^25 / (K (N + 1)) points each (option
 * "host_chunk": points per chunk).  On a failing point the status is the set's, *first_bad_index (may be NULL) = i in C
 * order over the whole lattice, and exactly the results in front of it are written, in both layouts: out[f][0..i) and
 * jac[f][d][0..i) (field-major), rows [0, i) of `out` and `jac` (fields-last); everything else is left as it was.  Shares
 * the sticky status words with the device form: finish device evaluations first. */
int interpn_hip_fields_eval_lattice_grad_host(interpn_hip_fields* fields, const void* const* axes, const size_t* axis_lens,
                                              size_t naxes, void* out, size_t out_stride, void* jac, size_t jac_stride,
                                              int layout, uint64_t* first_bad_index);
/* interpn_hip_fields_reserve_lattice for value-and-Jacobian calls: the per-field path's slice holds K (N + 1) rows.  The
 * same limit: a per-field evaluation with fields-last results holds two of the first handle's four blocks at a time, so for
 * THAT form the guarantee covers two concurrent streams.  A nearest set: INTERPN_HIP_ERR_UNSUPPORTED.  Synchronous. */
int interpn_hip_fields_reserve_lattice_grad(interpn_hip_fields* fields, const size_t* axis_lens, size_t naxes, int nstreams);
/* interpn_hip_fields_lattice_plan for a value-and-Jacobian call (no device; the same arguments, environment latches and
 * statuses), except that the nearest method has no gradient: INTERPN_HIP_ERR_UNSUPPORTED. */
int interpn_hip_fields_lattice_grad_plan(size_t elem_size, int method, size_t ndims, const size_t* dims, const size_t* axis_lens,
                                         size_t nfields, int layout, int* path, size_t* group, size_t* lds_bytes, size_t* npoints);

/* ------------------------------------------------------------------------------------------
 * Point-major observation points — the points as ONE array of shape (npoints, N), the layout of particle positions, ray
 * samples and scipy's `xi`, instead of N coordinate arrays.
 *
 * Definition  a block is a pointer `pts`, a count `npoints` and a `point_stride` >= ndims in ELEMENTS: coordinate d of
 *           point i is pts[i * point_stride + d].  point_stride > ndims covers buf[:, :3] of an (n, 4) array and records
 *           that carry other fields; elements d >= ndims of a row are never read.
 * Contract  the result of point i has exactly the bits of interpn_hip_eval_device on the N de-interleaved coordinate
 *           arrays, for every method, kind, N = 1..8, element type and fma flavour.  A failing point ("Unrepresentable
 *           coordinate value", regular grids) is reported as by interpn_hip_eval_device / _host, with the index of the
 *           point in the whole call.
 * Paths     FUSED (multilinear N = 2, 3 on a handle with a re-laid table): interpn::k_linear_points reads the rows
 *           directly — packed rows (point_stride == N) whose base is aligned to two elements as per-lane vector loads of
 *           the lane's own PPL * N consecutive elements (3-D f64: the wave's whole span through LDS, which measured
 *           faster), anything else element by element — and is otherwise the value
 *           kernel: one launch, no scratch, no allocation, capturable.
 *           DIRECT (N = 1 with point_stride == 1): the block is a coordinate array; interpn_hip_eval_device_ex, no copy.
 *           SPLIT (everything else: cubic, nearest, one_dim with a stride, N >= 4, handles without a table, option
 *           force_generic): interpn::k_split_points de-interleaves a slice (64 MiB of coordinates at most) into scratch and
 *           the slice goes through interpn_hip_eval_device_ex with all its paths and options.
 * Options   "points_path" = 0 automatic (fused where it exists), 1 fused or INTERPN_HIP_ERR_UNSUPPORTED, 2 split.
 *           "points_load" = 0 automatic (3-D f64: 2; else 1), 1 per-lane vector loads, 2 (3-D f64) the span through LDS, 3 element loads.
 *           "points_slice" (testing): points per slice of the split path.  Read-only "last_points_path"
 *           (INTERPN_HIP_POINTS_PATH_*; -1 before any).  interpn_hip_kernel_name reports "interpn::k_linear_points<...>"
 *           after a fused evaluation, the ordinary kernel otherwise.
 * Scratch   the split path works in one of the handle's scratch blocks under the rules of the lattice's expanded path:
 *           one block per concurrent stream, at most 4, allocated on first use unless INTERPN_HIP_EVAL_NO_ALLOC is given
 *           (then INTERPN_HIP_ERR_OUT_OF_MEMORY without one); interpn_hip_reserve_points provides them in advance; a
 *           stream under graph capture uses reserved blocks only.
 * Checks    before any device work, in this order: h NULL, point_stride < ndims (one_dim handles: < 1):
 *           INTERPN_HIP_ERR_INVALID_ARGUMENT; npoints == 0: INTERPN_HIP_OK whatever the other pointers are; pts or out
 *           NULL: INTERPN_HIP_ERR_INVALID_ARGUMENT; option points_path = 1 without a fused kernel:
 *           INTERPN_HIP_ERR_UNSUPPORTED.
 * ---------------------------------------------------------------------------------------- */
enum { INTERPN_HIP_POINTS_PATH_FUSED = 0, INTERPN_HIP_POINTS_PATH_SPLIT = 1, INTERPN_HIP_POINTS_PATH_DIRECT = 2 };
/* Asynchronous on `stream`.  `pts`, `out` (npoints elements): device.  `flags`: INTERPN_HIP_EVAL_NO_ALLOC.  *path_taken
 * (may be NULL): INTERPN_HIP_POINTS_PATH_*.  interpn_hip_finish reports a failing point. */
int interpn_hip_eval_points_device(interpn_hip_interp* h, const void* pts, size_t point_stride, size_t npoints, void* out,
                                   void* stream, unsigned flags, int* path_taken);
/* The same on host arrays, synchronous: chunks of 2^21 points (option "host_chunk"), the interleaved rows of a chunk
 * uploaded with one copy.  On a failing point the status is the handle's, exactly out[0..first_bad) is written and the rest
 * of `out` is left as it was.  Shares the sticky status word with the device form: finish device evaluations first. */
int interpn_hip_eval_points_host(interpn_hip_interp* h, const void* pts, size_t point_stride, size_t npoints, void* out);
/* Scratch blocks for split-path evaluations of up to `npoints` points on up to `nstreams` concurrent streams.
 * Synchronous.  A slice that the handle would sort or sweep takes a second block while it holds the first, and this call
 * sizes the first only.  interpn_hip_reserve counts EVERY block of the handle that is large enough, the slices' among them:
 * call it with the slice's point count and 2 * nstreams (one stream: nstreams + 1) behind this call.  A handle owns at
 * most 4 blocks and both calls clamp `nstreams` to 4: both levels can be reserved for two streams at most; with three
 * or four, some slices find no second block.  With one block per stream the slices are evaluated in place, under
 * INTERPN_HIP_EVAL_NO_ALLOC and under capture (which never sorts or sweeps); the results are the same bits. */
int interpn_hip_reserve_points(interpn_hip_interp* h, size_t npoints, int nstreams);

/* ------------------------------------------------------------------------------------------
 * Point-major gradients — value and d/dx of an (npoints, N) positions array in one pass, the gradient in the same layout:
 * what a differentiable model, a particle pusher, a ray marcher or a Newton step on a table holds and wants back.
 *
 * Definition  input block: `pts`, `npoints`, `point_stride` >= ndims in ELEMENTS as above; coordinate d of point i is
 *           pts[i * point_stride + d].  Value: `out`, npoints contiguous elements.  Gradient block: `grad` and a
 *           `grad_stride` >= ndims in ELEMENTS; component d of point i goes to grad[i * grad_stride + d].  Elements
 *           d >= ndims of a gradient row are never written and the last row's need not exist: g[:, :3] of an (n, 4) array
 *           is taken as it is.  `pts` and `grad` must not overlap.
 * Contract  multilinear handle: out[i] and grad[i, d] have exactly the bits interpn_hip_eval_grad_device gives on the N
 *           de-interleaved coordinate arrays; multicubic handle: exactly the bits of interpn_hip_eval_cubic_grad_device —
 *           for every kind, N = 1..8, f64 and f32, both fma flavours and both linearize_extrapolation settings.  One pair
 *           of entry points serves both methods: the handle's method picks.  Nearest and one_dim handles:
 *           INTERPN_HIP_ERR_UNSUPPORTED before any device work.
 * Paths     FUSED, multilinear N = 2, 3 on a handle with a re-laid table: interpn::k_linear_points_grad — the coordinate
 *           load of k_linear_points (option "points_load"), the arithmetic of k_linear_grad, and a gradient-row store in
 *           one of three forms: packed rows (grad_stride == N) whose base is aligned to two elements as per-lane vector
 *           stores of the lane's own PPL * N consecutive elements; (3-D f64, two points per lane) the wave's whole span
 *           through LDS as lane-contiguous 16-byte stores; anything else element by element.  Two points per lane
 *           need `out` aligned to two elements.  The kernel addresses a workgroup's rows by 32-bit offsets: it takes
 *           point_stride and grad_stride of up to 2^20 ELEMENTS each; longer rows go to the split path.
 *           FUSED, multicubic N = 2, 3 on a handle with its tiled table: interpn::k_cubic_points_grad — k_cubic_grad
 *           reading the point's row and storing to the point's gradient row, one point per lane.
 *           Either is one launch, uses no scratch, allocates nothing and is capturable.
 *           DIRECT (N = 1 with both strides 1): the blocks are a coordinate and a component array; the column form's
 *           launch, no copy.
 *           SPLIT (everything else: N = 1 with a stride, N >= 4, handles without a re-laid table, option force_generic,
 *           a multilinear handle with point_stride or grad_stride above 2^20 elements, "points_path" = 2): per slice interpn::k_split_points de-interleaves the rows into scratch, the column form's
 *           launch writes the value to `out` and the N components to scratch, interpn::k_join_grad interleaves them into
 *           the gradient rows.
 * Options   "points_path", "points_load", "points_slice" as above.  "points_store" = 0 automatic (the fastest measured
 *           form: 2 in 3-D f64 with two points per lane, 1 for other packed, aligned rows, else 3), 1 per-lane vector
 *           stores, 2 (3-D f64) the span through LDS, 3 element stores.  Read-only
 *           "last_points_path".  interpn_hip_kernel_name reports "interpn::k_linear_points_grad<...>" or
 *           "interpn::k_cubic_points_grad<...>" after a fused evaluation, the column form's kernel otherwise.
 * Scratch   the split path under the rules above; a slice needs N coordinate and N component arrays:
 *           interpn_hip_reserve_points_grad sizes blocks for that.
 * Checks    before any device work, in this order: h NULL: INTERPN_HIP_ERR_INVALID_ARGUMENT; a handle that is neither
 *           multilinear nor multicubic: INTERPN_HIP_ERR_UNSUPPORTED; point_stride < ndims or grad_stride < ndims:
 *           INTERPN_HIP_ERR_INVALID_ARGUMENT; npoints == 0: INTERPN_HIP_OK whatever the pointers are; pts, out or grad
 *           NULL: INTERPN_HIP_ERR_INVALID_ARGUMENT; a block whose bytes overflow size_t: INTERPN_HIP_ERR_INVALID_ARGUMENT;
 *           option points_path = 1 on a handle without a fused form, or with rows longer than the fused multilinear
 *           kernel takes: INTERPN_HIP_ERR_UNSUPPORTED.
 * Failing   regular grids: interpn_hip_finish reports the first failing index of the whole call (device form); the host
 * points    form writes exactly out[0..i) and gradient rows [0..i) and leaves everything else as it was.
 * ---------------------------------------------------------------------------------------- */
/* Asynchronous on `stream`.  `pts`, `out`, `grad`: device.  `flags`: INTERPN_HIP_EVAL_NO_ALLOC.  *path_taken (may be NULL):
 * INTERPN_HIP_POINTS_PATH_*. */
int interpn_hip_eval_points_grad_device(interpn_hip_interp* h, const void* pts, size_t point_stride, size_t npoints,
                                        void* out, void* grad, size_t grad_stride, void* stream, unsigned flags,
                                        int* path_taken);
/* The same on host arrays, synchronous: chunks like interpn_hip_eval_points_host, a chunk's rows uploaded with one copy,
 * the values and the gradient rows in front of the first failing point downloaded. */
int interpn_hip_eval_points_grad_host(interpn_hip_interp* h, const void* pts, size_t point_stride, size_t npoints,
                                      void* out, void* grad, size_t grad_stride);
/* Scratch blocks for split-path gradient evaluations of up to `npoints` points on up to `nstreams` concurrent streams.
 * Synchronous. */
int interpn_hip_reserve_points_grad(interpn_hip_interp* h, size_t npoints, int nstreams);

#ifdef __cplusplus
}
#endif

#endif /* INTERPN_HIP_H */
