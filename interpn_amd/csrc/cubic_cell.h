// The statements the multicubic kernels share, written once.
//
//   INTERPN_CUBIC_CLASS / _TT / _DIM_FILL / _LOCATE   a coordinate's cell on a regular grid: footprint origin, saturation
//                           class, linearized flag and local coordinate (multicubic/regular.rs:435-466, :356-360).  The
//                           whole step: k_cubic_regular (interpn_kernels.h), k_cubic_brick (cubic_brick.h), k_cubic3_column
//                           (cubic3_column.h) and the gradient cell below; its parts, around what is their own (k1_plain,
//                           the fast divisions, records instead of a CubicDimRegular): k_generic, k_generic_n
//                           (interpn_kernels.h), k_cubic_grad_n (cubic_grad.h), k_cubic_sweep (cubic_sweep.h) and
//                           k_lattice_axes (k_lattice.hip)
//   INTERPN_CUBIC_BRICK_PROLOGUE / _TILE_OFFSETS      k_cubic_brick, k_cubic_grad, k_cubic_points_grad on the tiled table
//                           (cubic_brick.h): the workgroup's LDS carve-up, axis staging and lane indices; a point's 16
//                           table offsets from its cell
//   INTERPN_CUBIC_GRAD_CELL / _GRAD_SIGNED            what k_cubic_grad (cubic_grad.h) and k_cubic_points_grad
//                           (points_grad.h) do between their own coordinate loads and stores: locate, gather, the value
//                           and the partial derivatives of every plane, the combine over dimension 2; a component's sign
//
// The shared statements are macros, not functions, for the reason linear_cell.h gives: an inlined function is optimised on
// its own before it is inlined, and the kernels built from it differ from the ones built from the same statements written
// in place (the locate step of k_cubic_grad as a __forceinline__ function with reference out-parameters: SGPR count
// changed in 80 of 88 instantiations, about 7 % of the assembly lines different, branch structure included).  Expanded in
// place the statements give the machine code of the former copies, byte for byte (profiles/cubic_cell_resources.md).
// Each macro names what it expects in scope and what it declares; the element type T is the kernels' own, and so are the
// template parameters N, RECT, FMA, SI, SJ and the arguments `a` of the three brick kernels.
//
// This header holds macros only and includes nothing, so that interpn_kernels.h (which cubic_brick.h builds on) can use the
// locate step: what a macro names has to be declared where it is expanded, not here.
#pragma once

// Class from floc.  FLOC = regular_floc's result (an integer-valued float, = iloc + 1), START / STEP / NNODES the
// dimension's grid.  Declares l (the footprint's first node: iloc clamped to 0 .. n - 4), sat, outside and
// index_one_loc (the coordinate of node l + 1).  All comparisons are on floc, which is exact for |floc| < 2^63; beyond
// 2^53 neighbouring integers coincide in f64 but every threshold involved (-1, 0, n - 3) is far below that:
// iloc < -1 <=> floc < 0; iloc == -1 <=> floc == 0; iloc > n - 3 <=> floc > n - 2; iloc == n - 3 <=> floc == n - 2.
#define INTERPN_CUBIC_CLASS(FLOC, START, STEP, NNODES) \
  const T nn = (T)(NNODES);                                                                                  \
  const int l = clamp_loc<T>((FLOC) - (T)1, (NNODES) - 4);  /* regular.rs:440-442 */                         \
  int sat;                                                                                                   \
  bool outside;                                                                                              \
  if ((FLOC) < (T)0) { sat = kSatLow; outside = true; }  /* regular.rs:445-466 */                            \
  else if ((FLOC) == (T)0) { sat = kSatLow; outside = false; }                                               \
  else if ((FLOC) > nn - (T)2) { sat = kSatHigh; outside = true; }                                           \
  else if ((FLOC) == nn - (T)2) { sat = kSatHigh; outside = false; }                                         \
  else { sat = kSatNone; outside = false; }                                                                  \
  const T index_one_loc = mul_add<false>((STEP), (T)(l + 1), (START));  /* regular.rs:356-360, never fused */

// Behind INTERPN_CUBIC_CLASS: the node's local coordinate from TT = (x - index_one_loc) / step (an expression).
#define INTERPN_CUBIC_TT(TT) (sat == kSatLow ? -(TT) : (sat == kSatHigh ? (TT) - (T)1 : (TT)))

// Behind INTERPN_CUBIC_CLASS: fills sat, linear and tt of DIM (a CubicDimRegular<T>) from TT.
#define INTERPN_CUBIC_DIM_FILL(DIM, TT, LINEARIZE) \
  (DIM).sat = sat;                                  \
  (DIM).linear = (outside && (LINEARIZE)) ? 1 : 0;  \
  (DIM).tt = INTERPN_CUBIC_TT(TT);

// The whole step for the coordinate X (a variable): declares floc, t and what INTERPN_CUBIC_CLASS declares, fills DIM,
// and clears OK (a bool) for a coordinate the reference panics on.
#define INTERPN_CUBIC_LOCATE(X, START, STEP, NNODES, LINEARIZE, DIM, OK) \
  T floc;                                                                                 \
  OK &= regular_floc<T>((X), (START), (STEP), &floc);  /* multicubic/regular.rs:435-438 */ \
  OK &= floc != (T)-9223372036854775808.0;  /* `- 1` would overflow isize */              \
  INTERPN_CUBIC_CLASS(floc, START, STEP, NNODES)                                          \
  const T t = ((X) - index_one_loc) / (STEP);                                             \
  INTERPN_CUBIC_DIM_FILL(DIM, t, LINEARIZE)

// The workgroup's prologue.  Declares smem_raw, lds_data and lds_off (ONE region, used first for the offset transpose
// (u32) and then for the data transposes (T)), DMA, kRegion, lds_axes, axis_base (the axis image the rectilinear locate
// reads: LDS or L2), lane, me, group, goff, rsrc and lds_wave.
#define INTERPN_CUBIC_BRICK_PROLOGUE() \
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];                                              \
  typedef T __attribute__((may_alias)) lds_T;                                                                           \
  lds_T* lds_data = reinterpret_cast<lds_T*>(smem_raw);                                                                 \
  lds_u32* lds_off = reinterpret_cast<lds_u32*>(smem_raw);                                                              \
  constexpr bool DMA = cubic_dma<T, SI, SJ>();                                                                          \
  constexpr size_t kRegion = cubic_lds_region<T, SI, SJ>();                                                             \
  unsigned char* lds_axes = smem_raw + kRegion;                                                                         \
  if (RECT && a.ax.use_lds) stage_axes<T, N>(a.ax, lds_axes);                                                           \
  const unsigned char* axis_base = (RECT && a.ax.use_lds) ? lds_axes : a.ax.image;                                      \
  const unsigned lane = threadIdx.x;                                                                                    \
  const unsigned me = lane & 15;                                                                                        \
  const unsigned group = lane >> 4;                                                                                     \
  /* the offset matrix of a group lives inside the SAME bytes as its data matrix (both are private to the group's */    \
  /* wave): indexed with the data matrix' group stride */                                                               \
  const unsigned goff = group * (unsigned)(16 * kCubRow * sizeof(T) / 4);                                               \
  const __amdgpu_buffer_rsrc_t rsrc = table_rsrc(a.bricks, a.table_bytes);                                              \
  /* LDS byte address of this wave's tile image (LDS-DMA gather), in a scalar register */                               \
  const unsigned lds_wave = (unsigned)__builtin_amdgcn_readfirstlane(                                                   \
      (int)((unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem_raw + (lane >> 6) * cubic_dma_image<T>()));

// A point's table offsets.  Expects loc[] (dims 0 and 1), pbase (the element offset of the point's first plane) and the
// prologue; declares toff[16], byte offsets.  LDS-DMA form (steps 1,1: tile index = cell): toff[q], q < sizeof(T) = the
// piece instruction q of a plane's DMA has this lane fetch, piece c of point p (cubic_brick.h::dma_issue_plane), from the
// owners' tile offsets by shuffle.  Other steps: the 16 footprint elements of this lane's point go to LDS, and the lane
// reads back element `me` of its group's 16 points (every lane takes part, dead lanes with the offsets of a valid point).
#define INTERPN_CUBIC_TILE_OFFSETS() \
  unsigned toff[16];                                                                                                    \
  if constexpr (DMA) {                                                                                                  \
    constexpr unsigned PP = (unsigned)sizeof(T);  /* 16-byte pieces per tile; 64 / PP points per DMA instruction */     \
    const unsigned wl = lane & 63u;                                                                                     \
    const unsigned tb = (pbase + (unsigned)(loc[0] * (int)a.nbj + loc[1]) * 16u) * (unsigned)sizeof(T);                 \
    _Pragma("unroll")                                                                                                   \
    for (int q = 0; q < (int)PP; ++q) {                                                                                 \
      const unsigned p = ((unsigned)q * 64u + wl) / PP;                                                                 \
      const unsigned c = ((wl & (PP - 1u)) - cubic_dma_rot<T>(p)) & (PP - 1u);                                          \
      toff[q] = (unsigned)__shfl((int)tb, (int)p) + c * 16u;                                                            \
    }                                                                                                                   \
  } else {                                                                                                              \
    _Pragma("unroll")                                                                                                   \
    for (int e = 0; e < 16; ++e) {                                                                                      \
      int bi, oi, bj, oj;                                                                                               \
      tile_coord<SI>(loc[0], e >> 2, &bi, &oi);                                                                         \
      tile_coord<SJ>(loc[1], e & 3, &bj, &oj);                                                                          \
      lds_off[goff + e * kCubRow + me] =                                                                                \
          (pbase + ((unsigned)(bi * (int)a.nbj + bj) * 16u) + (unsigned)(oi * 4 + oj)) * (unsigned)sizeof(T);           \
    }                                                                                                                   \
    wave_sync();                                                                                                        \
    _Pragma("unroll")                                                                                                   \
    for (int r = 0; r < 16; ++r) toff[r] = lds_off[goff + me * kCubRow + r];                                            \
    wave_sync();                                                                                                        \
  }

// The gradient cell, N = 2, 3.  X = the point's coordinate along `d` (an expression in d, evaluated once per dimension;
// a dead lane's must be that of a valid point: it takes part in the gathers' exchanges).  A point that is LIVE and that a
// regular grid cannot place reports INDEX.  Expects the prologue.  Declares dim[N], loc[N], width[N] (the spacing t was
// divided by), res = the value and g[N] = the partial derivatives in tt, which INTERPN_CUBIC_GRAD_SIGNED and one division finish.
// Planes in the reference's order (dim 2 ascending); per plane the value, d/dx0 and d/dx1 after dims 0 and 1.
#define INTERPN_CUBIC_GRAD_CELL(X, LIVE, INDEX) \
  typedef typename CubicDimSel<T, RECT>::type DimT;                                                                     \
  constexpr int NP = N == 2 ? 1 : 4;  /* planes of a point */                                                           \
  DimT dim[N];                                                                                                          \
  int loc[N];                                                                                                           \
  T width[N];                                                                                                           \
  bool ok = true;                                                                                                       \
  _Pragma("unroll")                                                                                                     \
  for (int d = 0; d < N; ++d) {                                                                                         \
    const T x = (X);                                                                                                    \
    if constexpr (RECT) {                                                                                               \
      const Axis<T> ax = make_axis<T, N>(a.ax, axis_base, d);                                                           \
      loc[d] = cubic_rect_locate<T>(ax, x, a.linearize, /*fma_linear=*/false, dim[d]);  /* multicubic/rectilinear.rs:366-408 */ \
      width[d] = cubic_rect_width<T>(ax.g, loc[d], dim[d].sat);                                                         \
    } else {                                                                                                            \
      INTERPN_CUBIC_LOCATE(x, a.start[d], a.step[d], a.n[d], a.linearize, dim[d], ok)                                   \
      loc[d] = l;                                                                                                       \
      width[d] = a.step[d];                                                                                             \
    }                                                                                                                   \
  }                                                                                                                     \
  if (!RECT && !ok && (LIVE)) atomicMin(a.first_bad, (unsigned long long)(INDEX));                                      \
  unsigned pbase = 0;  /* element offsets here, bytes in LDS */                                                         \
  if constexpr (N == 3) pbase = (unsigned)loc[2] * a.plane_stride[2];                                                   \
  INTERPN_CUBIC_TILE_OFFSETS()                                                                                          \
  auto delta_of = [&](int k) -> unsigned {  /* byte offset of plane k along dim 2 */                                    \
    if constexpr (N == 3) return (unsigned)k * a.plane_stride[2] * (unsigned)sizeof(T);                                 \
    else return 0u;                                                                                                     \
  };                                                                                                                    \
  T sv[NP], s0[NP], s1[NP];                                                                                             \
  if constexpr (DMA) dma_issue_plane<T>(rsrc, toff, delta_of(0), lds_wave);                                             \
  _Pragma("unroll")                                                                                                     \
  for (int k = 0; k < NP; ++k) {                                                                                        \
    T v[16];                                                                                                            \
    if constexpr (DMA) {                                                                                                \
      dma_take_tile<T>(lds_wave, lane & 63u, v);                                                                        \
      if (k + 1 < NP) dma_issue_plane<T>(rsrc, toff, delta_of(k + 1), lds_wave);                                        \
    } else {                                                                                                            \
      grad_gather_tile<T>(rsrc, toff, delta_of(k), lds_data, group, me, v);                                             \
    }                                                                                                                   \
    grad_reduce_tile<T, RECT, FMA>(v, dim, sv[k], s0[k], s1[k]);                                                        \
  }                                                                                                                     \
  T res, g[N];                                                                                                          \
  if constexpr (N == 2) {                                                                                               \
    res = sv[0];                                                                                                        \
    g[0] = s0[0];                                                                                                       \
    g[1] = s1[0];                                                                                                       \
  } else {                                                                                                              \
    cubic_node_vd<RECT, FMA, T>(sv[0], sv[1], sv[2], sv[3], dim[2], res, g[2]);                                         \
    g[0] = cubic_node_sel<RECT, FMA, T>(s0[0], s0[1], s0[2], s0[3], dim[2]);                                            \
    g[1] = cubic_node_sel<RECT, FMA, T>(s1[0], s1[1], s1[2], s1[3], dim[2]);                                            \
  }

// Behind INTERPN_CUBIC_GRAD_CELL: g[D] with the sign of its class (an expression; tt runs against x in a Low class).
// Component D of the gradient is this divided by width[D], ONE division, which the kernels write where they store.
#define INTERPN_CUBIC_GRAD_SIGNED(D) (dim[D].sat == kSatLow ? -g[D] : g[D])
