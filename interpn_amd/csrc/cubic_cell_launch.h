// Host side of the three kernels on the tiled multicubic table (k_cubic_brick, k_cubic_grad, k_cubic_points_grad): the
// arguments they share, the LDS size, and the dispatch over the kernels' template parameters.  A kernel is named by a
// trait:
//   struct K {
//     static constexpr const char* name;                      what GridDesc::tag reports
//     template <typename T, int N> using Args;                the kernel's argument struct
//     template <typename T, int N, bool RECT, bool FMA, int SI, int SJ>
//     static auto kernel();                                   the instantiation's address
//   };
// Args has bricks, table_bytes, first_bad, npts, linearize, start, step, n, ax, nbj and plane_stride; everything else is
// the kernel's own.
#pragma once

#include "cubic_brick.h"

namespace interpn {

// The fused gradient kernels run where the handle keeps the tiled table they gather from (N = 2, 3; a 4-D handle's tiles
// are left to the runtime-N kernel).
inline bool cubic_grad_fused_applies(const GridDesc& g) {
  return g.method == kCubic && g.bricks && !g.cfg.force_generic && (g.ndims == 2 || g.ndims == 3);
}

template <typename K, typename T, int N, bool RECT, bool FMA>
hipError_t cubic_cell_launch_steps(const GridDesc& g, const typename K::template Args<T, N>& a, size_t lds, unsigned blocks,
                                   hipStream_t stream) {
  const int si = g.brick_step[0], sj = g.brick_step[1];
#define CUBIC_GO(SI, SJ)                                                                                              \
  do {                                                                                                                \
    g.tag.set(K::name, {N, RECT, FMA, SI, SJ}, 0b00110u);                                                             \
    hipLaunchKernelGGL((K::template kernel<T, N, RECT, FMA, SI, SJ>()), dim3(blocks), dim3(kBlock), lds, stream, a);  \
  } while (0)
  if (si == 4 && sj == 4) CUBIC_GO(4, 4);
  else if (si == 2 && sj == 4) CUBIC_GO(2, 4);
  else if (si == 2 && sj == 2) CUBIC_GO(2, 2);
  else if (si == 1 && sj == 4) CUBIC_GO(1, 4);
  else if (si == 1 && sj == 1) CUBIC_GO(1, 1);
  else return hipErrorInvalidValue;
#undef CUBIC_GO
  return hipGetLastError();
}

// Fills what the three argument structs share and launches `blocks` workgroups; the caller has set the kernel's own
// members.
template <typename K, typename T, int N>
hipError_t cubic_cell_launch(const GridDesc& g, typename K::template Args<T, N>& a, size_t npts, unsigned long long* first_bad,
                             unsigned blocks, hipStream_t stream) {
  a.bricks = static_cast<const T*>(g.bricks);
  {
    unsigned nb[2];
    size_t bytes = 0;
    cubic_tile_geometry(g, g.brick_step[0], g.brick_step[1], nb, &bytes);
    a.table_bytes = (unsigned)bytes;  // < 4 GiB by construction (maybe_build_cubic_tiles)
  }
  a.first_bad = first_bad;
  a.npts = npts;
  a.linearize = g.linearize;
  for (int d = 0; d < N; ++d) {
    a.start[d] = (T)g.start[d];
    a.step[d] = (T)g.step[d];
    a.n[d] = g.n[d];
    a.plane_stride[d] = 0;
  }
  a.nbj = g.brick_nb[1];
  // table[plane index (dims 2..N-1, C order)][bi][bj][16]
  unsigned acc = g.brick_nb[0] * g.brick_nb[1] * 16u;
  for (int d = N - 1; d >= 2; --d) {
    a.plane_stride[d] = acc;
    acc *= (unsigned)g.n[d];
  }
  const bool dma = g.brick_step[0] == 1 && g.brick_step[1] == 1;  // cubic_brick.h::cubic_dma
  size_t lds = dma ? (size_t)(kBlock / 64) * cubic_dma_image<T>() : (size_t)kBlock * kCubRow * (sizeof(T) > 4 ? sizeof(T) : 4);
  a.ax.use_lds = 0;
  a.ax.image = nullptr;
  a.ax.image_bytes = 0;
  if (g.kind == kRectilinear) lds += fill_axis_args<T, N>(g, a.ax);
  if (g.kind == kRegular)
    return g.fma ? cubic_cell_launch_steps<K, T, N, false, true>(g, a, lds, blocks, stream)
                 : cubic_cell_launch_steps<K, T, N, false, false>(g, a, lds, blocks, stream);
  return g.fma ? cubic_cell_launch_steps<K, T, N, true, true>(g, a, lds, blocks, stream)
               : cubic_cell_launch_steps<K, T, N, true, false>(g, a, lds, blocks, stream);
}

}  // namespace interpn
