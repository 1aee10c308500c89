// One multilinear cell per point, N = 2, 3, on the re-laid table a handle already has: what k_linear_grad (linear_grad.h),
// k_linear_points (linear_points.h) and k_linear_points_grad (points_grad.h) do between their own loads and stores.
//
//   INTERPN_CELL_PROLOGUE   the workgroup's prologue: the gather's LDS carve-up and the rectilinear axes (lane registers,
//                           LDS or L2)
//   INTERPN_CELL_SEARCH     a point's cell: t, width and loc per dimension on regular or rectilinear grids, the first_bad
//                           report
//   INTERPN_CELL_VALUE3 / _GRAD3   N = 3: the cell's corners by linear_brick.h's quad gather (bricks of every layout), the
//                           value tree; the three gradient components
//   INTERPN_CELL_VALUE2 / _GRAD2   N = 2: the corners by k_linear2_brick's lane-pair gather, the value; the two components
//   INTERPN_POINTS_LOAD     the coordinate load of the two point-major kernels (PointsLoad, points_forms.h)
//
// Cell search, t and the value are the value kernels' operations, so a value has eval's bits.  The gradient comes from
// the same 2^N corner values (DESIGN.md "Gradients" holds the definition the kernels are tested against bit for bit):
//   W[c']   = V[c' | 1 << d] - V[c']           one subtraction per corner pair
//   s       = W reduced over e != d, ascending e, with the reference's lerp(t[e], y0, y1)
//   grad[d] = s / h[d]                          IEEE division; h = steps[d], or x1 - x0 of the point's cell
//
// The shared statements are macros, not functions, and that is deliberate.  The compiler optimises an inlined function on
// its own before it inlines it, and the kernels it then builds differ from the ones it builds from the same statements
// written in place: by -18 to +8 VGPRs, and some instantiations that sit just below an occupancy step cross it
// however the function is cut (even a kernel whose whole unchanged body is moved into one inlined function does).  Expanded
// in place the statements give the machine code of the three former copies, byte for byte (profiles/linear_cell_resources.md
// has both comparisons).  Each macro names what it expects in scope and what it declares; the template parameters T, N,
// RECT, FMA, SI, SJ, PPL, AXR, CELL, the kernel's arguments `a` and `lane` = threadIdx.x are the kernels' own.
#pragma once

#include "linear_brick.h"
#include "points_forms.h"

namespace interpn {

// the reference's interpolation step (multilinear/regular.rs:378-385)
template <bool FMA, typename T>
__device__ __forceinline__ T cell_lerp(T t, T y0, T y1) {
  const T dy = y1 - y0;
  return mul_add<FMA>(t, dy, y0);
}

// swap with the neighbouring lane (lane ^ 1): quad_perm [1,0,3,2]
__device__ __forceinline__ unsigned lane_swap1(unsigned v) {
  return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true);
}
__device__ __forceinline__ float lane_swap1(float v) { return __uint_as_float(lane_swap1(__float_as_uint(v))); }
__device__ __forceinline__ double lane_swap1(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = lane_swap1((unsigned)b), hi = lane_swap1((unsigned)(b >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// Dynamic LDS in front of the axis image.  N == 3: [pieces][offsets] as in k_linear_brick; N == 2: none (the gather is a
// lane-pair swap)
template <typename T, int N>
constexpr size_t cell_gather_lds() {
  return N == 3 ? (size_t)kBlock * kPieceRow * sizeof(typename LeafVec<T, 2>::type) + (size_t)kBlock * 16 : 0;
}

// Declares P, smem_raw, lds_piece, lds_off (N == 3: [pieces][offsets] as in k_linear_brick; N == 2: the axes alone, the
// gather is a lane-pair swap), la (AXR != 0: the axes in lane registers) and axis_base (the axis image the other searches
// read: LDS or L2).
#define INTERPN_CELL_PROLOGUE() \
  typedef typename LeafVec<T, 2>::type P;                                                                             \
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];                                            \
  /* N == 3: [pieces][offsets][axes] as in k_linear_brick; N == 2: the axes alone (the gather is a lane-pair swap) */ \
  constexpr size_t kGatherLds = cell_gather_lds<T, N>();                                                              \
  P* lds_piece = reinterpret_cast<P*>(smem_raw);                                                                      \
  lds_u32* lds_off = reinterpret_cast<lds_u32*>(smem_raw + kBlock * kPieceRow * sizeof(P));                           \
  unsigned char* lds_axes = smem_raw + kGatherLds;                                                                    \
  LaneAxes<T, N> la;                                                                                                  \
  if constexpr (RECT && AXR != 0) {                                                                                   \
    la = load_lane_axes<T, N, AXR>(a.ax);                                                                             \
  } else if (RECT && a.ax.use_lds) {                                                                                  \
    stage_axes<T, N>(a.ax, lds_axes);                                                                                 \
  }                                                                                                                   \
  const unsigned char* axis_base = (RECT && AXR == 0 && a.ax.use_lds) ? lds_axes : a.ax.image;

// Point (X)[N] -> t[N], width[N], loc[N], which it declares.  CELL_R / X0_R / X1_R: the point's rows of what
// lane_axes_locate found (AXR != 0; unread otherwise).  A point that is LIVE and that the grid cannot place reports INDEX.
#define INTERPN_CELL_SEARCH(X, CELL_R, X0_R, X1_R, LIVE, INDEX) \
  T t[N], width[N];                                                                                 \
  int loc[N];                                                                                       \
  bool ok = true;                                                                                   \
  _Pragma("unroll")                                                                                 \
  for (int d = 0; d < N; ++d) {                                                                     \
    const T x = (X)[d];                                                                             \
    if (RECT) {                                                                                     \
      T x0, x1;                                                                                     \
      int l;                                                                                        \
      if constexpr (AXR != 0) {                                                                     \
        l = (CELL_R)[d];                                                                            \
        x0 = (X0_R)[d];                                                                             \
        x1 = (X1_R)[d];                                                                             \
      } else {                                                                                      \
        const Axis<T> ax = make_axis<T, N>(a.ax, axis_base, d);                                     \
        l = axis_cell<T>(ax, x, &x0, &x1);  /* multilinear/rectilinear.rs:353-370, :310-311 */      \
      }                                                                                             \
      const T step = x1 - x0;                                                                       \
      t[d] = (x - x0) / step;  /* rectilinear.rs:310-313 */                                         \
      width[d] = step;                                                                              \
      loc[d] = l;                                                                                   \
    } else {                                                                                        \
      T floc;                                                                                       \
      ok &= regular_floc<T>(x, a.start[d], a.step[d], &floc);  /* multilinear/regular.rs:415-418 */ \
      const int l = clamp_loc<T>(floc, a.n[d] - 2);  /* regular.rs:420-422 */                       \
      const T izl = mul_add<FMA>(a.step[d], (T)l, a.start[d]);  /* regular.rs:334-337 */            \
      t[d] = (x - izl) / a.step[d];  /* regular.rs:339 */                                           \
      width[d] = a.step[d];                                                                         \
      loc[d] = l;                                                                                   \
    }                                                                                               \
  }                                                                                                 \
  if (!RECT && !ok && (LIVE)) atomicMin(a.first_bad, (unsigned long long)(INDEX));

// N == 3, behind INTERPN_CELL_SEARCH: gathers the cell `c` (every lane of a quad takes part, dead lanes too) and
// VAL = its value.
#define INTERPN_CELL_VALUE3(VAL) \
  typedef BrickGeom<T, CELL> Geom;                                                                                      \
  const unsigned q = lane & 3;                                                                                          \
  const unsigned quad = lane >> 2;                                                                                      \
  const unsigned bk = (unsigned)loc[2] / (unsigned)Geom::SK;                                                            \
  const unsigned kpart = bk * (unsigned)Geom::ELEMS + ((unsigned)loc[2] - bk * (unsigned)Geom::SK);                     \
  _Pragma("unroll")                                                                                                     \
  for (int p = 0; p < 4; ++p)                                                                                           \
    lds_off[(quad * 4 + p) * 4 + q] = brick_piece<T, SI, SJ, CELL>(a.nbj, a.nbk, loc[0], loc[1], kpart, p >> 1, p & 1); \
  wave_sync();                                                                                                          \
  const uint4 toff = *reinterpret_cast<const uint4*>(&lds_off[(quad * 4 + q) * 4]);                                     \
  const Cell<T> c = gather_cell<T>(a.bricks, toff, 0u, lds_piece, quad, q);                                             \
  /* value: the tree of k_linear_brick (i first, k last; multilinear/regular.rs:347-403) */                             \
  T r[2];                                                                                                               \
  _Pragma("unroll")                                                                                                     \
  for (int dk = 0; dk < 2; ++dk) {                                                                                      \
    const T c0 = cell_lerp<FMA>(t[0], c.v[0][0][dk], c.v[1][0][dk]);                                                    \
    const T c1 = cell_lerp<FMA>(t[0], c.v[0][1][dk], c.v[1][1][dk]);                                                    \
    r[dk] = cell_lerp<FMA>(t[1], c0, c1);                                                                               \
  }                                                                                                                     \
  VAL = cell_lerp<FMA>(t[2], r[0], r[1]);

// ... and G0, G1, G2 = the gradient's components.
#define INTERPN_CELL_GRAD3(G0, G1, G2) \
  /* d/dx0: differences along i, reduced over j then k */                                       \
  T s[2];                                                                                       \
  _Pragma("unroll")                                                                             \
  for (int dk = 0; dk < 2; ++dk)                                                                \
    s[dk] = cell_lerp<FMA>(t[1], c.v[1][0][dk] - c.v[0][0][dk], c.v[1][1][dk] - c.v[0][1][dk]); \
  G0 = cell_lerp<FMA>(t[2], s[0], s[1]) / width[0];                                             \
  /* d/dx1: differences along j, reduced over i then k */                                       \
  _Pragma("unroll")                                                                             \
  for (int dk = 0; dk < 2; ++dk)                                                                \
    s[dk] = cell_lerp<FMA>(t[0], c.v[0][1][dk] - c.v[0][0][dk], c.v[1][1][dk] - c.v[1][0][dk]); \
  G1 = cell_lerp<FMA>(t[2], s[0], s[1]) / width[1];                                             \
  /* d/dx2: differences along k, reduced over i then j */                                       \
  _Pragma("unroll")                                                                             \
  for (int dj = 0; dj < 2; ++dj)                                                                \
    s[dj] = cell_lerp<FMA>(t[0], c.v[0][dj][1] - c.v[0][dj][0], c.v[1][dj][1] - c.v[1][dj][0]); \
  G2 = cell_lerp<FMA>(t[1], s[0], s[1]) / width[2];

// N == 2, behind INTERPN_CELL_SEARCH: gathers the rows row0, row1 (both lanes of a pair take part) and VAL = the cell's
// value.
#define INTERPN_CELL_VALUE2(VAL) \
  /* the lane-pair gather of k_linear2_brick: brick (bi = i, bj = j / SJ2), two row pieces per point */ \
  constexpr unsigned KW2 = 64 / sizeof(T), SJ2 = KW2 - 1, EL2 = 2 * KW2;                                \
  const unsigned q = lane & 1;                                                                          \
  const unsigned bj = (unsigned)loc[1] / SJ2;                                                           \
  const unsigned mine = ((unsigned)loc[0] * a.nbj + bj) * EL2 + ((unsigned)loc[1] - bj * SJ2);          \
  const unsigned theirs = lane_swap1(mine);                                                             \
  const unsigned off0 = (q == 0 ? mine : theirs) + q * KW2;                                             \
  const unsigned off1 = (q == 0 ? theirs : mine) + q * KW2;                                             \
  const P p0 = *reinterpret_cast<const P*>(a.bricks + off0);                                            \
  const P p1 = *reinterpret_cast<const P*>(a.bricks + off1);                                            \
  const P keep = q == 0 ? p0 : p1;                                                                      \
  const P send = q == 0 ? p1 : p0;                                                                      \
  P recv;                                                                                               \
  recv.x = lane_swap1(send.x);                                                                          \
  recv.y = lane_swap1(send.y);                                                                          \
  const P row0 = q == 0 ? keep : recv;  /* v(i, j), v(i, j+1) */                                        \
  const P row1 = q == 0 ? recv : keep;  /* row i+1 */                                                   \
  const T c0 = cell_lerp<FMA>(t[0], row0.x, row1.x);                                                    \
  const T c1 = cell_lerp<FMA>(t[0], row0.y, row1.y);                                                    \
  VAL = cell_lerp<FMA>(t[1], c0, c1);

// ... and G0, G1 = the gradient's components.
#define INTERPN_CELL_GRAD2(G0, G1) \
  G0 = cell_lerp<FMA>(t[1], row1.x - row0.x, row1.y - row0.y) / width[0]; \
  G1 = cell_lerp<FMA>(t[0], row0.y - row0.x, row1.y - row1.x) / width[1];

// The coordinate load of the point-major kernels into xin[PPL][N], which comes preset (points that are not live[h] keep
// it).  Expects lds_piece, TV (a naturally aligned two-element vector of T) and wl = the lane's index in its wave, WAVE of
// the workgroup.  The two kernels address their rows differently (64-bit element indices; 32-bit offsets from the
// iteration's first row), so the addresses are arguments.  a.load (PointsLoad, launch-uniform):
//   kPointsLoadElem   one element load per coordinate, element (ROW_OFF) + d from ROW_BASE, both of which may name the
//                     point `h` of the lane: any stride, any alignment
//   kPointsLoadWide   stride == N, base aligned to two elements: the lane's own PPL * N contiguous elements as two-element
//                     vector loads from vector WIDE_OFF of WIDE_BASE on (3-D f64, PPL = 2: three 16-byte loads of the
//                     lane's 48 bytes)
//   kPointsLoadLds    3-D f64 with PPL = 2, where the wave has all its 64 * PPL points (SPAN_WHOLE): the wave's 3072-byte
//                     span from SPAN as three lane-contiguous 16-byte loads into the wave's own part of the piece exchange
//                     area, read back 48 bytes per lane (no LDS beyond what the gather has; waves of the ragged tail take
//                     the wide form)
#define INTERPN_POINTS_LOAD(WAVE, SPAN_WHOLE, SPAN, WIDE_BASE, WIDE_OFF, ROW_BASE, ROW_OFF) \
  constexpr bool kCanWide = (PPL * N) % 2 == 0;                                                                  \
  constexpr bool kCanLds = N == 3 && sizeof(T) == 8 && PPL == 2;                                                 \
  bool loaded = false;                                                                                           \
  if constexpr (kCanLds) {                                                                                       \
    if (a.load == kPointsLoadLds && (SPAN_WHOLE)) {  /* wave-uniform */                                          \
      typedef T V16 __attribute__((ext_vector_type(2), aligned(16)));                                            \
      /* the wave's quads' rows of the piece area: 16 quads x 4 rows x kPieceRow slots, idle until the gather */ \
      P* mine = lds_piece + (size_t)(WAVE) * 16 * 4 * kPieceRow;                                                 \
      static_assert(16 * 4 * kPieceRow >= 64 * PPL * N / 2, "a wave's span fits its part of the piece area");    \
      const V16* src = reinterpret_cast<const V16*>(SPAN);                                                       \
      V16 r[3];                                                                                                  \
      _Pragma("unroll")                                                                                          \
      for (int k = 0; k < 3; ++k) r[k] = stream_load(src + k * 64 + wl);                                         \
      _Pragma("unroll")                                                                                          \
      for (int k = 0; k < 3; ++k) *reinterpret_cast<V16*>(mine + k * 64 + wl) = r[k];                            \
      wave_sync();                                                                                               \
      _Pragma("unroll")                                                                                          \
      for (int k = 0; k < 3; ++k) {                                                                              \
        const P w = mine[wl * 3 + k];                                                                            \
        xin[(2 * k) / N][(2 * k) % N] = w.x;                                                                     \
        xin[(2 * k + 1) / N][(2 * k + 1) % N] = w.y;                                                             \
      }                                                                                                          \
      wave_sync();                                                                                               \
      loaded = true;                                                                                             \
    }                                                                                                            \
  }                                                                                                              \
  if constexpr (kCanWide) {                                                                                      \
    if (!loaded && a.load != kPointsLoadElem && live[PPL - 1]) {                                                 \
      const TV* src = reinterpret_cast<const TV*>(WIDE_BASE);                                                    \
      _Pragma("unroll")                                                                                          \
      for (int k = 0; k < PPL * N / 2; ++k) {                                                                    \
        const TV w = stream_load(src + ((WIDE_OFF) + k));                                                        \
        xin[(2 * k) / N][(2 * k) % N] = w.x;                                                                     \
        xin[(2 * k + 1) / N][(2 * k + 1) % N] = w.y;                                                             \
      }                                                                                                          \
      loaded = true;                                                                                             \
    }                                                                                                            \
  }                                                                                                              \
  if (!loaded) {  /* any stride or alignment, and the batch's ragged tail */                                     \
    _Pragma("unroll")                                                                                            \
    for (int h = 0; h < PPL; ++h)                                                                                \
      if (live[h]) {                                                                                             \
        const T* rows = ROW_BASE;                                                                                \
        _Pragma("unroll")                                                                                        \
        for (int d = 0; d < N; ++d) xin[h][d] = stream_load(rows + ((ROW_OFF) + d));                             \
      }                                                                                                          \
  }

}  // namespace interpn
