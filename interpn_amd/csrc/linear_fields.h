// Multi-field multilinear interpolation: K value grids on one grid, one pass over the points
// (include/interpn_hip.h, "Field sets").  N = 2, 3; regular and rectilinear; f64 and f32.
//
// Table.  One 128-byte line holds the 2^N corners of ONE cell for P = 128 / (2^N sizeof(T)) consecutive
// fields (f64: P = 2 for N = 3, 4 for N = 2; f32: 4 and 8).  Inside a field's 2^N values bit d of the
// corner index is the offset along dimension d, so dimension 0's pair is innermost and a 16-byte piece
// holds the operands of the reference's first reduction (f64: the dim-0 pair; f32: the dim-0 pairs of
// both dim-1 rows).  The ceil(K / P) lines of a cell follow each other, cells are in C order, fields
// beyond K in the last line are zero.  Size: prod(n_d - 1) * ceil(K / P) * 128 bytes.
//
// Kernel.  One lane per point reads its N coordinates once and computes the cell and t[N] with the
// device functions of the single-field kernels (regular_floc / clamp_loc / mul_add<FMA>, axis_cell),
// so these bits cannot differ from a single handle's.  The wave then shares {first line of the cell,
// t[N]} of its 64 points through LDS and walks the line groups g < ceil(K / P) (a wave-uniform loop):
// 8 lanes x 16 bytes fetch one point's line, so one load instruction covers 8 whole lines and the 8 in
// flight per wave cover its 64 points.  Each field's reduction tree runs in the reference's order —
// dimension 0 first, the last dimension last (src/multilinear/regular.rs:347-403): the levels inside a
// piece are local to the lane, the others take the partner lane's node through DPP (partners differ in
// bit 0 or 1 of the lane number, i.e. sit in one quad).  Every node sees the operands the reference
// gives it: y0 = the lower corner's node, dy = upper - y0, t.mul_add(dy, y0).  Results go through LDS
// so that every field's row is stored as one contiguous 64-element run per wave.
#pragma once

#include "rect_args.h"

namespace interpn {

template <typename T, int N>
struct FieldsLayout {
  static constexpr int kLineBytes = 128;
  static constexpr int EPP = 16 / (int)sizeof(T);        // elements of a 16-byte piece
  static constexpr int LB = sizeof(T) == 8 ? 1 : 2;      // dimensions reduced inside a piece
  static constexpr int XB = N - LB;                      // dimensions reduced across lanes
  static constexpr int P = 8 >> XB;                      // fields per line = 128 / (2^N sizeof(T))
  static constexpr int EPL = kLineBytes / (int)sizeof(T);
  // LDS of one wave: first line of the cell (u32) and t[N] of its 64 points, then P result rows
  static constexpr unsigned kWaveLds = 64u * 4u + (unsigned)(N + P) * 64u * (unsigned)sizeof(T);
  static_assert(N == 2 || N == 3, "fused fields: N = 2, 3");
};

template <typename T, int N>
struct FieldsArgs {
  const unsigned char* table;
  const T* obs[N];
  T* out;
  size_t out_stride;  // elements between the rows of two fields
  unsigned long long* first_bad;
  size_t npts;
  int nfields;
  unsigned groups;      // lines per cell: ceil(nfields / P)
  unsigned cstride[N];  // lines between neighbouring cells along each dimension (C order, times `groups`)
  T start[N];
  T step[N];
  int n[N];
  AxisArgs<T, N> ax;    // rectilinear grids only
};

// The partner lane's value, partner = lane ^ X for X = 1, 2: a quad permutation (DPP), no LDS traffic.
template <int X>
__device__ __forceinline__ int quad_xor_word(int v) {
  static_assert(X == 1 || X == 2, "partners inside a quad");
  constexpr int ctrl = X == 1 ? 0xB1 : 0x4E;  // quad_perm [1,0,3,2] / [2,3,0,1]
  return __builtin_amdgcn_update_dpp(0, v, ctrl, 0xF, 0xF, false);
}
template <int X>
__device__ __forceinline__ float quad_xor(float v) { return __int_as_float(quad_xor_word<X>(__float_as_int(v))); }
template <int X>
__device__ __forceinline__ double quad_xor(double v) {
  return __hiloint2double(quad_xor_word<X>(__double2hiint(v)), quad_xor_word<X>(__double2loint(v)));
}

// One node of the tree: multilinear/regular.rs:378-385 (the same expression at every level).
template <bool FMA, typename T>
__device__ __forceinline__ T fields_node(T t, T lo, T hi) {
  const T y0 = lo;
  const T dy = hi - y0;
  return mul_add<FMA>(t, dy, y0);
}

template <int K, bool FMA, typename T>
__device__ __forceinline__ T fields_cross_level(T r, T t, int piece) {
  const T other = quad_xor<(1 << K)>(r);
  const bool upper = ((piece >> K) & 1) != 0;
  return fields_node<FMA, T>(t, upper ? other : r, upper ? r : other);
}

// What k_linear_fields and k_linear_fields_points (linear_fields_points.h) do between their own coordinate loads and result
// stores, as statements expanded in place (macros for the reason linear_cell.h gives: an inlined function is optimised on
// its own first, and the kernel built from it is not the kernel built from the statements).  The template parameters T, N,
// RECT, FMA, the layout L = FieldsLayout<T, N>, the 16-byte piece type V and the kernel's arguments `a` (table, groups,
// cstride, start, step, n, ax, first_bad) are the kernels' own.
//
// INTERPN_FIELDS_PROLOGUE(WAVE_LDS)  declares smem_raw, axbase (the rectilinear axes: LDS or L2), wave, lane, wlds = the
//     wave's WAVE_LDS bytes of LDS, s_line and s_t at its start, piece, psub.
#define INTERPN_FIELDS_PROLOGUE(WAVE_LDS) \
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];    \
  unsigned lds_axes = 0;                                                      \
  const unsigned char* axbase = nullptr;                                      \
  if constexpr (RECT) {                                                       \
    axbase = a.ax.image;                                                      \
    if (a.ax.use_lds) {                                                       \
      stage_axes<T, N>(a.ax, smem_raw);                                       \
      lds_axes = (a.ax.image_bytes + 15u) & ~15u;                             \
      axbase = smem_raw;                                                      \
    }                                                                         \
  }                                                                           \
  const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);  \
  unsigned char* wlds = smem_raw + lds_axes + (unsigned)wave * (WAVE_LDS);    \
  lds_u32* s_line = reinterpret_cast<lds_u32*>(wlds);                         \
  T* s_t = reinterpret_cast<T*>(wlds + 256);                                  \
  const int piece = lane & 7, psub = lane >> 3;

// INTERPN_FIELDS_LOCATE(X, LIVE, INDEX)  the point of this lane: X is its coordinate along `d` (an expression in d; lanes
//     behind the batch give a harmless one), a LIVE point the grid cannot place reports INDEX.  Shares {first line of the
//     cell, t[N]} of the wave's 64 points through s_line / s_t and declares lines[8], the lines this lane fetches pieces of.
#define INTERPN_FIELDS_LOCATE(X, LIVE, INDEX) \
  T t[N];                                                                                                        \
  unsigned line = 0;                                                                                             \
  bool ok = true;                                                                                                \
  _Pragma("unroll")                                                                                              \
  for (int d = 0; d < N; ++d) {                                                                                  \
    int loc;                                                                                                     \
    if constexpr (RECT) {                                                                                        \
      const T x = (X);                                                                                           \
      const Axis<T> ax = make_axis<T, N>(a.ax, axbase, d);                                                       \
      T x0, x1;                                                                                                  \
      loc = axis_cell<T>(ax, x, &x0, &x1);  /* rectilinear.rs:353-370, :310-311 */                               \
      const T step = x1 - x0;                                                                                    \
      t[d] = (x - x0) / step;               /* rectilinear.rs:310-313 */                                         \
    } else {                                                                                                     \
      const T x = (X);                                                                                           \
      T floc;                                                                                                    \
      ok &= regular_floc<T>(x, a.start[d], a.step[d], &floc);  /* regular.rs:415-418 */                          \
      loc = clamp_loc<T>(floc, a.n[d] - 2);                    /* regular.rs:420-422 */                          \
      const T index_zero_loc = mul_add<FMA>(a.step[d], (T)loc, a.start[d]);  /* regular.rs:334-339 */            \
      t[d] = (x - index_zero_loc) / a.step[d];                                                                   \
    }                                                                                                            \
    line += (unsigned)loc * a.cstride[d];                                                                        \
  }                                                                                                              \
  if (!ok && (LIVE)) atomicMin(a.first_bad, (unsigned long long)(INDEX));                                        \
  s_line[lane] = line;                                                                                           \
  _Pragma("unroll")                                                                                              \
  for (int d = 0; d < N; ++d) s_t[d * 64 + lane] = t[d];                                                         \
  wave_sync();                                                                                                   \
  unsigned lines[8];                                                                                             \
  _Pragma("unroll")                                                                                              \
  for (int j = 0; j < 8; ++j) lines[j] = s_line[j * 8 + psub];

// INTERPN_FIELDS_GROUP(G, DST)  line group G of the wave's 64 points: 8 lanes x 16 bytes fetch one point's line, every
//     field's tree runs in the reference's order, and the lane that ends up with field `fl` of the line for point `p` of
//     the wave stores it to DST (an LDS lvalue in fl and p).
#define INTERPN_FIELDS_GROUP(G, DST) \
  V v[8];                                                                                                                 \
  _Pragma("unroll")                                                                                                       \
  for (int j = 0; j < 8; ++j)                                                                                             \
    v[j] = *reinterpret_cast<const V*>(a.table + ((size_t)lines[j] + (G)) * L::kLineBytes + (unsigned)piece * 16u);       \
  _Pragma("unroll")                                                                                                       \
  for (int j = 0; j < 8; ++j) {                                                                                           \
    const int p = j * 8 + psub;                                                                                           \
    T tt[N];                                                                                                              \
    _Pragma("unroll")                                                                                                     \
    for (int d = 0; d < N; ++d) tt[d] = s_t[d * 64 + p];                                                                  \
    T r;                                                                                                                  \
    if constexpr (L::LB == 1) {                                                                                           \
      r = fields_node<FMA, T>(tt[0], v[j][0], v[j][1]);                                                                   \
    } else {                                                                                                              \
      const T r0 = fields_node<FMA, T>(tt[0], v[j][0], v[j][1]);                                                          \
      const T r1 = fields_node<FMA, T>(tt[0], v[j][2], v[j][3]);                                                          \
      r = fields_node<FMA, T>(tt[1], r0, r1);                                                                             \
    }                                                                                                                     \
    if constexpr (L::XB >= 1) r = fields_cross_level<0, FMA, T>(r, tt[L::LB], piece);                                     \
    if constexpr (L::XB >= 2) r = fields_cross_level<1, FMA, T>(r, tt[L::LB + 1], piece);                                 \
    const int fl = piece >> L::XB;                                                                                        \
    if ((piece & ((1 << L::XB) - 1)) == 0) DST = r;                                                                       \
  }

template <typename T, int N, bool RECT, bool FMA>
__global__ void __launch_bounds__(kBlock) k_linear_fields(const FieldsArgs<T, N> a) {
  typedef FieldsLayout<T, N> L;
  typedef T V __attribute__((ext_vector_type(L::EPP)));
  INTERPN_FIELDS_PROLOGUE(L::kWaveLds);
  T* s_res = s_t + N * 64;

  // whole workgroups iterate together: every lane of a wave stays active (the exchanges below need it);
  // lanes behind the batch evaluate a harmless coordinate and only their stores are masked
  for (size_t base = (size_t)blockIdx.x * kBlock; base < a.npts; base += (size_t)gridDim.x * kBlock) {
    const size_t i = base + threadIdx.x;
    const bool live = i < a.npts;
    INTERPN_FIELDS_LOCATE(live ? stream_load(a.obs[d] + i) : (RECT ? (T)0 : a.start[d]), live, i);
    const size_t wbase = base + (size_t)wave * 64;
    for (unsigned g = 0; g < a.groups; ++g) {
      INTERPN_FIELDS_GROUP(g, s_res[fl * 64 + p]);
      wave_sync();
#pragma unroll
      for (int fl = 0; fl < L::P; ++fl) {
        const size_t f = (size_t)g * L::P + fl;
        if (f < (size_t)a.nfields && wbase + lane < a.npts) stream_store(a.out + f * a.out_stride + wbase + lane, s_res[fl * 64 + lane]);
      }
      wave_sync();
    }
  }
}

// The table from the field-major `vals` (field f = the C-ordered grid at vals + f * field_stride): one thread per
// table element, plain vector stores.
template <int N>
struct FieldsBuildDims {
  unsigned ncell[N];   // n_d - 1
  size_t stride[N];    // element stride of dimension d in a field's grid
};

template <typename T, int N>
__global__ void __launch_bounds__(kBlock) k_fields_build(const T* __restrict__ vals, size_t field_stride, int nfields, unsigned groups,
                                                         const FieldsBuildDims<N> dims, T* __restrict__ table, size_t total) {
  typedef FieldsLayout<T, N> L;
  const size_t nthreads = (size_t)gridDim.x * kBlock;
  for (size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += nthreads) {
    const size_t ln = e / L::EPL;
    const unsigned within = (unsigned)(e % L::EPL);
    const unsigned corner = within & ((1u << N) - 1u);
    const size_t f = (ln % groups) * L::P + (within >> N);
    size_t cell = ln / groups;
    size_t idx = 0;
#pragma unroll
    for (int d = N - 1; d >= 0; --d) {
      const size_t loc = cell % dims.ncell[d];
      cell /= dims.ncell[d];
      idx += (loc + ((corner >> d) & 1u)) * dims.stride[d];
    }
    table[e] = f < (size_t)nfields ? vals[f * field_stride + idx] : (T)0;
  }
}

}  // namespace interpn
