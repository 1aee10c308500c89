// Point-major observation points: coordinate d of point i is pts[i * stride + d] (an (n, N) array, or rows of a wider
// record), evaluated without de-interleaving them first.
//
//   k_linear_points<T, N, RECT, FMA, SI, SJ, PPL, AXR, CELL>   N = 2, 3 multilinear on the re-laid table the handle already
//       has: the shared cell body of linear_cell.h without its gradient part.  Cell search, t, the gather (3-D bricks of
//       every layout, the 2-D lane-pair gather) and the value tree are the value kernels' statements, so a result has the
//       bits of interpn_hip_eval_device on the de-interleaved columns.  The coordinate load (PointsArgs::load,
//       launch-uniform: element, wide or through LDS) is INTERPN_POINTS_LOAD of linear_cell.h, which k_linear_points_grad
//       expands too, here with 64-bit element indices; the store of the values is the kernel's own.
//   k_split_points<T>   de-interleaves a slice of the block into N coordinate arrays (everything the fused kernel does not
//       take then goes through the ordinary kernels): the rows are read contiguously, each coordinate array is written
//       contiguously, through an LDS tile.
//   k_points_bad_begin / _end   one lane each, around a slice that does not start at point 0: the first-failing-index word
//       counts from the start of the whole call.
#pragma once

#include "linear_cell.h"

namespace interpn {

template <typename T, int N>
struct PointsArgs {
  const T* bricks;
  const T* pts;
  size_t stride;  // elements from point to point, >= N
  T* out;
  unsigned long long* first_bad;
  size_t npts;
  int load;  // PointsLoad
  T start[N];
  T step[N];
  int n[N];
  AxisArgs<T, N> ax;
  unsigned nbj, nbk;  // N == 3: bricks along j and k; N == 2: nbj = bricks along j
  unsigned iters;     // kBlock-wide iterations per workgroup
};

template <typename T, int N, bool RECT, bool FMA, int SI, int SJ, int PPL, int AXR = 0, int CELL = 0>
__global__ void __launch_bounds__(kBlock) k_linear_points(const PointsArgs<T, N> a) {
  static_assert(N == 2 || N == 3, "fused point-major kernel: N = 2, 3");
  static_assert(CELL == 0 || (CELL == 2 && N == 3 && sizeof(T) == 4 && SI == 1 && SJ == 1), "2 x 4 x 4 bricks: 3-D f32");
  INTERPN_CELL_PROLOGUE();
  const unsigned lane = threadIdx.x;
  const size_t nslots = (a.npts + PPL - 1) / PPL;
  const size_t first = (size_t)blockIdx.x * a.iters * kBlock;
  typedef T TV __attribute__((ext_vector_type(2)));  // naturally aligned: vector accesses of the wide form and of `out`
  for (unsigned it = 0; it < a.iters; ++it) {
    // every lane runs every iteration (dead lanes still fetch pieces for their quad / pair)
    const size_t s0 = first + (size_t)it * kBlock + lane;
    if (s0 - lane >= nslots) break;  // block-uniform
    const size_t i0 = s0 * PPL;
    T xin[PPL][N];
    bool live[PPL];
#pragma unroll
    for (int h = 0; h < PPL; ++h) live[h] = i0 + h < a.npts;
#pragma unroll
    for (int h = 0; h < PPL; ++h)
#pragma unroll
      for (int d = 0; d < N; ++d) xin[h][d] = RECT ? (T)0 : a.start[d];
    const unsigned wl = lane & 63u;
    const size_t wave_p0 = (s0 - wl) * PPL;  // the wave's first point; it has 64 * PPL of them
    INTERPN_POINTS_LOAD(lane >> 6, wave_p0 + 64 * PPL <= a.npts, a.pts + wave_p0 * N, a.pts + i0 * N, 0, a.pts + (i0 + h) * a.stride, 0);
    int cell_r[PPL][N];
    T x0_r[PPL][N], x1_r[PPL][N];
    if constexpr (RECT && AXR != 0) lane_axes_locate<T, N, PPL, AXR>(a.ax, la, xin, cell_r, x0_r, x1_r);
    T resv[PPL];
#pragma unroll
    for (int h = 0; h < PPL; ++h) {
      INTERPN_CELL_SEARCH(xin[h], cell_r[h], x0_r[h], x1_r[h], live[h], i0 + h);
      if constexpr (N == 3) {
        INTERPN_CELL_VALUE3(resv[h]);
      } else {
        INTERPN_CELL_VALUE2(resv[h]);
      }
    }
    if constexpr (PPL >= 2) {
      if (live[PPL - 1]) {
        TV v;
#pragma unroll
        for (int h = 0; h < PPL; ++h) v[h] = resv[h];
        stream_store(reinterpret_cast<TV*>(a.out + i0), v);
      } else {
#pragma unroll
        for (int h = 0; h < PPL; ++h)
          if (live[h]) stream_store(a.out + i0 + h, resv[h]);
      }
    } else if (live[0]) {
      stream_store(a.out + i0, resv[0]);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
template <typename T>
struct SplitArgs {
  const T* pts;
  size_t stride;
  size_t count;
  int ndims;
  T* dst[kMaxDims];
};

// One workgroup per kBlock points: their rows are kBlock * stride consecutive elements.
template <typename T>
__global__ void __launch_bounds__(kBlock) k_split_points(const SplitArgs<T> a) {
  __shared__ T tile[kMaxDims][kBlock + 1];
  const size_t p0 = (size_t)blockIdx.x * kBlock;
  const size_t here = a.count - p0 < (size_t)kBlock ? a.count - p0 : (size_t)kBlock;
  const T* rows = a.pts + p0 * a.stride;
  if (a.stride > kSplitTileStride) {  // rows of long records: a lane per point, nothing to coalesce (launch-uniform)
    if (threadIdx.x < here)
      for (int d = 0; d < a.ndims; ++d) a.dst[d][p0 + threadIdx.x] = stream_load(rows + threadIdx.x * a.stride + d);
    return;
  }
  const unsigned stride = (unsigned)a.stride;
  const unsigned span = (unsigned)here * stride;
  for (unsigned e = threadIdx.x; e < span; e += kBlock) {
    const unsigned p = e / stride;
    const unsigned d = e - p * stride;
    // elements d >= ndims of a row are somebody else's (the last row's may not even exist): never read
    if (d < (unsigned)a.ndims) tile[d][p] = stream_load(rows + e);
  }
  __syncthreads();
  if (threadIdx.x < here)
    for (int d = 0; d < a.ndims; ++d) a.dst[d][p0 + threadIdx.x] = tile[d][threadIdx.x];
}

__global__ void k_points_bad_begin(unsigned long long* word, unsigned long long* saved) {
  *saved = *word;
  *word = kNoBadIndex;
}

__global__ void k_points_bad_end(unsigned long long* word, const unsigned long long* saved, unsigned long long begin) {
  unsigned long long w = *word;
  if (w != kNoBadIndex) w += begin;
  const unsigned long long s = *saved;
  *word = s < w ? s : w;
}

}  // namespace interpn
