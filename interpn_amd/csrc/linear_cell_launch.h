// Host side of the three kernels built on linear_cell.h (k_linear_grad, k_linear_points, k_linear_points_grad): which
// handles they take, the arguments they share, the points-per-lane and coordinate-load rules, and the dispatch over the
// kernels' template parameters.  A kernel is named by a trait:
//   struct K {
//     static constexpr const char* name;                      what GridDesc::tag reports
//     template <typename T, int N> using Args;                the kernel's argument struct
//     template <typename T, int N, bool RECT, bool FMA, int SI, int SJ, int PPL, int AXR, int CELL>
//     static auto kernel();                                   the instantiation's address
//   };
// Args has bricks, first_bad, npts, start, step, n, ax, nbj, nbk and iters; everything else is the kernel's own.
#pragma once

#include <cstdint>
#include <initializer_list>

#include "linear_cell.h"

namespace interpn {

// The kernels run where the handle keeps the table they gather from: the 2-D bricks, or 3-D bricks of any of the
// layouts 11 / 12 / 22 / f32 2 x 4 x 4.  (3-D handles never have the 4-D cell bricks.)
inline bool linear_cell_applies(const GridDesc& g) {
  if (g.method != kLinear || !g.bricks || g.cfg.force_generic) return false;
  if (g.ndims == 2) return true;
  return g.ndims == 3 && g.brick_cell != 1;
}

template <typename T>
inline bool aligned2(const void* p) { return (reinterpret_cast<uintptr_t>(p) % (2 * sizeof(T))) == 0; }

// Two points per lane (vector accesses of the streams a lane owns two consecutive elements of) when every one of
// `streams` is aligned to 2 * sizeof(T); the handle's `ppl` option = 1 forces the scalar form, as for the value kernels.
template <typename T>
inline bool cell_two_points(const GridDesc& g, std::initializer_list<const void*> streams) {
  bool aligned = true;
  for (const void* p : streams) aligned = aligned && aligned2<T>(p);
  return aligned && g.cfg.ppl != 1;
}

// The coordinate load of the point-major kernels (INTERPN_POINTS_LOAD).  Packed rows whose base is aligned to two
// elements: vector loads of the lane's own elements (every lane's first element is then aligned too: PPL * N is even, or
// the form is not compiled); anything else: element loads.
template <typename T, int N>
inline int points_load_form(const GridDesc& g, const T* pts, size_t stride, bool two) {
  int load = kPointsLoadElem;
  if (stride == (size_t)N && aligned2<T>(pts)) {
    load = kPointsLoadWide;
    // 3-D f64 with two points per lane: the wave's span through LDS instead, the faster of the two forms (1.25 against
    // 1.51 ms per 1e8 points on 64^3); option points_load = 1 keeps the per-lane loads
    if (N == 3 && sizeof(T) == 8 && two && g.cfg.points_load != kPointsLoadWide) load = kPointsLoadLds;
  }
  if (g.cfg.points_load == 3) load = kPointsLoadElem;  // testing / measurements: element loads whatever the layout
  return load;
}

template <typename K, typename T, int N, bool RECT, bool FMA, int PPL, int AXR>
hipError_t cell_launch_steps(const GridDesc& g, const typename K::template Args<T, N>& a, size_t lds, unsigned blocks,
                             hipStream_t stream) {
#define CELL_GO(SI, SJ, CELL)                                                                                              \
  do {                                                                                                                     \
    g.tag.set(K::name, {N, RECT, FMA, SI, SJ, PPL, AXR, CELL}, 0b00000110u);                                               \
    hipLaunchKernelGGL((K::template kernel<T, N, RECT, FMA, SI, SJ, PPL, AXR, CELL>()), dim3(blocks), dim3(kBlock), lds,   \
                       stream, a);                                                                                         \
    return hipGetLastError();                                                                                              \
  } while (0)
  if constexpr (N == 2) {
    CELL_GO(1, 1, 0);
  } else {
    if constexpr (sizeof(T) == 4) {
      if (g.brick_cell == 2) CELL_GO(1, 1, 2);
    }
    const int si = g.brick_step[0], sj = g.brick_step[1];
    if (si == 1 && sj == 1) CELL_GO(1, 1, 0);
    if (si == 1 && sj == 2) CELL_GO(1, 2, 0);
    CELL_GO(2, 2, 0);
  }
#undef CELL_GO
}

template <typename K, typename T, int N, int PPL>
hipError_t cell_launch_kind(const GridDesc& g, typename K::template Args<T, N>& a, size_t axis_lds, hipStream_t stream) {
  const size_t lds = cell_gather_lds<T, N>();
  const int axr = lane_axes_mode(g);  // axes in lanes (lane_axes.h) or 0 = LDS / L2 search
  a.iters = brick_iters(g, a.npts, PPL, /*setup=*/g.kind != kRectilinear ? 0 : (axr == 0 ? 2 : 1));
  const size_t nslots = (a.npts + PPL - 1) / PPL;
  const size_t per_block = (size_t)kBlock * a.iters;
  const unsigned blocks = (unsigned)((nslots + per_block - 1) / per_block);
  if (g.kind == kRegular)
    return g.fma ? cell_launch_steps<K, T, N, false, true, PPL, 0>(g, a, lds, blocks, stream)
                 : cell_launch_steps<K, T, N, false, false, PPL, 0>(g, a, lds, blocks, stream);
  if (axr == 2)
    return g.fma ? cell_launch_steps<K, T, N, true, true, PPL, 2>(g, a, lds, blocks, stream)
                 : cell_launch_steps<K, T, N, true, false, PPL, 2>(g, a, lds, blocks, stream);
  if (axr == 3)
    return g.fma ? cell_launch_steps<K, T, N, true, true, PPL, 3>(g, a, lds, blocks, stream)
                 : cell_launch_steps<K, T, N, true, false, PPL, 3>(g, a, lds, blocks, stream);
  if (axr == 1)
    return g.fma ? cell_launch_steps<K, T, N, true, true, PPL, 1>(g, a, lds, blocks, stream)
                 : cell_launch_steps<K, T, N, true, false, PPL, 1>(g, a, lds, blocks, stream);
  return g.fma ? cell_launch_steps<K, T, N, true, true, PPL, 0>(g, a, lds + axis_lds, blocks, stream)
               : cell_launch_steps<K, T, N, true, false, PPL, 0>(g, a, lds + axis_lds, blocks, stream);
}

// Fills what the three argument structs share and launches; the caller has set the kernel's own members.
template <typename K, typename T, int N>
hipError_t cell_launch(const GridDesc& g, typename K::template Args<T, N>& a, size_t npts, unsigned long long* first_bad,
                       bool two, hipStream_t stream) {
  a.bricks = static_cast<const T*>(g.bricks);
  a.first_bad = first_bad;
  a.npts = npts;
  for (int d = 0; d < N; ++d) {
    a.start[d] = (T)g.start[d];
    a.step[d] = (T)g.step[d];
    a.n[d] = g.n[d];
  }
  a.nbj = g.brick_nb[1];
  a.nbk = N == 3 ? g.brick_nb[2] : 1u;
  a.ax.use_lds = 0;
  a.ax.image = nullptr;
  a.ax.image_bytes = 0;
  size_t axis_lds = 0;
  // the 2-D kernel has no other LDS use: its axis image may take the wide budget, as in k_linear2_brick
  if (g.kind == kRectilinear) axis_lds = fill_axis_args<T, N>(g, a.ax, /*big_lds=*/N == 2, /*records=*/true);
  if (two) return cell_launch_kind<K, T, N, 2>(g, a, axis_lds, stream);
  return cell_launch_kind<K, T, N, 1>(g, a, axis_lds, stream);
}

}  // namespace interpn
