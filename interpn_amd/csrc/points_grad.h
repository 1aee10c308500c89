// Point-major value AND gradient: coordinate d of point i is pts[i * stride + d], component d of its gradient goes to
// grad[i * gstride + d] (an (n, N) positions array in, an (n, N) gradient array out), without de-interleaving the
// points first or interleaving the components afterwards.
//
//   k_linear_points_grad<T, N, RECT, FMA, SI, SJ, PPL, AXR, CELL>   N = 2, 3 multilinear on the re-laid table the handle
//       already has.  The coordinate load is the one k_linear_points expands (all three forms, PointsGradArgs::load);
//       prologue, cell search, t, the gather, the value tree and the gradient arithmetic are the shared cell body of
//       linear_cell.h, so `out` and `grad` have the bits of interpn_hip_eval_grad_device on the de-interleaved columns.
//       The kernel's own are the 32-bit row addressing, the two pins and the gradient-row store (PointsGradArgs::store,
//       launch-uniform):
//         kPointsStoreElem   one element store per component: any stride, any alignment; also the ragged tail
//         kPointsStoreWide   gstride == N, base aligned to two elements: the lane's own PPL * N contiguous elements as
//                            two-element vector stores (the mirror of kPointsLoadWide)
//         kPointsStoreLds    3-D f64 with PPL = 2: every lane writes its 48 bytes into the wave's own part of the piece
//                            exchange area (idle after the iteration's last gather), the wave stores its 3072-byte span
//                            as three lane-contiguous 16-byte stores (no LDS beyond what the gather has; waves of the
//                            ragged tail take the wide form)
//       Elements d >= N of a gradient row are never written.
//       A workgroup's rows are addressed by 32-bit offsets from the iteration's uniform first point (the launcher keeps
//       both strides at or below kPointsGradMaxStride), and two empty `asm volatile` statements pin values where they
//       are written: the lane index inside the iteration (what is derived from it is otherwise loop invariant, hoisted
//       and held in registers across the iteration) and the first point's results in front of the second point's gather
//       (otherwise their arithmetic is sunk behind it and the first cell stays live).  With them every instantiation
//       keeps the occupancy step of its k_linear_grad counterpart (tests/test_points_grad_cpu.py).  Measured, they buy no
//       speed: the un-pinned build (INTERPN_POINTS_GRAD_NO_PINS below) ran 1 - 4 % faster per 1e8 points in the four
//       instantiations that were timed (3-D f64 1.696 against 1.762 ms) and level at 1e6; they stay for the occupancy
//       requirement, which covers all 180 instantiations.  DESIGN.md section 14.
//   k_cubic_points_grad<T, N, RECT, FMA, SI, SJ>   N = 2, 3 on the tiled table of a cubic handle: k_cubic_grad with the
//       coordinates read from the point's row and the N components stored to the point's gradient row; one point per
//       lane, element accesses, or for N = 2 with packed aligned rows (`vec2`) one two-element vector access each.
//       Between that load and those stores it is the gradient cell of cubic_cell.h (INTERPN_CUBIC_BRICK_PROLOGUE,
//       INTERPN_CUBIC_GRAD_CELL), the statements k_cubic_grad expands, so `out` and `grad` have that kernel's bits.
//   k_join_grad<T>   the split path's last step, the mirror of k_split_points: interleaves N component arrays into the
//       gradient rows through an LDS tile (contiguous reads of every array, contiguous writes of the rows that skip
//       columns d >= N); rows longer than kSplitTileStride elements: a lane per point.
#pragma once

#include "cubic_grad.h"
#include "linear_cell.h"

// The pins of k_linear_points_grad (see above).  INTERPN_POINTS_GRAD_NO_PINS builds the kernel without them, for
// `make variant` measurements only (DESIGN.md section 14 has the figures); the product is never built that way.
#ifdef INTERPN_POINTS_GRAD_NO_PINS
#define INTERPN_POINTS_GRAD_PIN(x) ((void)0)
#else
#define INTERPN_POINTS_GRAD_PIN(x) asm volatile("" : "+v"(x))
#endif

namespace interpn {

template <typename T, int N>
struct PointsGradArgs {
  const T* bricks;
  const T* pts;
  size_t stride;  // elements from point to point, >= N
  T* out;
  T* grad;
  size_t gstride;  // elements from gradient row to gradient row, >= N
  unsigned long long* first_bad;
  size_t npts;
  int load;   // PointsLoad
  int store;  // PointsStore
  T start[N];
  T step[N];
  int n[N];
  AxisArgs<T, N> ax;
  unsigned nbj, nbk;  // N == 3: bricks along j and k; N == 2: nbj = bricks along j
  unsigned iters;     // kBlock-wide iterations per workgroup
};

template <typename T, int N, bool RECT, bool FMA, int SI, int SJ, int PPL, int AXR = 0, int CELL = 0>
__global__ void __launch_bounds__(kBlock) k_linear_points_grad(const PointsGradArgs<T, N> a) {
  static_assert(N == 2 || N == 3, "fused point-major gradient kernel: N = 2, 3");
  static_assert(CELL == 0 || (CELL == 2 && N == 3 && sizeof(T) == 4 && SI == 1 && SJ == 1), "2 x 4 x 4 bricks: 3-D f32");
  INTERPN_CELL_PROLOGUE();
  const unsigned lane = threadIdx.x;
  const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(lane >> 6));
  const size_t nslots = (a.npts + PPL - 1) / PPL;
  const size_t first = (size_t)blockIdx.x * a.iters * kBlock;
  typedef T TV __attribute__((ext_vector_type(2)));  // naturally aligned: vector accesses of the wide forms and of `out`
  for (unsigned it = 0; it < a.iters; ++it) {
    // every lane runs every iteration (dead lanes still fetch pieces for their quad / pair)
    // per lane everything is a 32-bit offset from the iteration's uniform first point p0 (the launcher keeps the strides
    // below 2^20 elements): uniform bases, one offset register per access
    const size_t slot0 = first + (size_t)it * kBlock;
    if (slot0 >= nslots) break;  // block-uniform
    const size_t p0 = slot0 * PPL;
    const unsigned left = a.npts - p0 < (size_t)kBlock * PPL ? (unsigned)(a.npts - p0) : (unsigned)kBlock * PPL;  // >= 1
    // (the lane's offsets are loop invariants: pinned inside the iteration, or they are hoisted and held in registers across it)
    unsigned lane_in = lane;
    INTERPN_POINTS_GRAD_PIN(lane_in);
    const unsigned lp = lane_in * PPL;  // the lane's first point, from p0
    T xin[PPL][N];
    bool live[PPL];
#pragma unroll
    for (int h = 0; h < PPL; ++h) live[h] = lp + h < left;
#pragma unroll
    for (int h = 0; h < PPL; ++h)
#pragma unroll
      for (int d = 0; d < N; ++d) xin[h][d] = RECT ? (T)0 : a.start[d];
    const unsigned wl = lane & 63u;
    const unsigned wave_lp = wave * 64u * PPL;  // the wave's first point, from p0; it has 64 * PPL of them
    INTERPN_POINTS_LOAD(wave, wave_lp + 64 * PPL <= left, a.pts + (p0 + wave_lp) * N, a.pts + p0 * N, lp * N / 2, a.pts + p0 * a.stride,
                        (lp + h) * (unsigned)a.stride);
    int cell_r[PPL][N];
    T x0_r[PPL][N], x1_r[PPL][N];
    if constexpr (RECT && AXR != 0) lane_axes_locate<T, N, PPL, AXR>(a.ax, la, xin, cell_r, x0_r, x1_r);
    T resv[PPL], gradv[N][PPL];
#pragma unroll
    for (int h = 0; h < PPL; ++h) {
      INTERPN_CELL_SEARCH(xin[h], cell_r[h], x0_r[h], x1_r[h], live[h], p0 + lp + h);
      if constexpr (N == 3) {
        INTERPN_CELL_VALUE3(resv[h]);
        INTERPN_CELL_GRAD3(gradv[0][h], gradv[1][h], gradv[2][h]);
      } else {
        INTERPN_CELL_VALUE2(resv[h]);
        INTERPN_CELL_GRAD2(gradv[0][h], gradv[1][h]);
      }
      if (h + 1 < PPL) {  // this point's results are complete here: they are not left to be computed behind the next gather
        INTERPN_POINTS_GRAD_PIN(resv[h]);
#pragma unroll
        for (int d = 0; d < N; ++d) INTERPN_POINTS_GRAD_PIN(gradv[d][h]);
      }
    }
    // ---- the value store of k_linear_points
    unsigned lane_out = lane;
    INTERPN_POINTS_GRAD_PIN(lane_out);
    const unsigned lq = lane_out * PPL;  // lp again, computed here
    if constexpr (PPL >= 2) {
      if (live[PPL - 1]) {
        TV v;
#pragma unroll
        for (int h = 0; h < PPL; ++h) v[h] = resv[h];
        stream_store(reinterpret_cast<TV*>(a.out + p0) + lane_out, v);
      } else {
#pragma unroll
        for (int h = 0; h < PPL; ++h)
          if (live[h]) stream_store(a.out + p0 + (lq + h), resv[h]);
      }
    } else if (live[0]) {
      stream_store(a.out + p0 + lq, resv[0]);
    }
    // ---- the gradient-row store: element e of the lane's PPL * N is component e % N of its point e / N
    bool stored = false;
    if constexpr (kCanLds) {
      if (a.store == kPointsStoreLds && wave_lp + 64 * PPL <= left) {  // wave-uniform
        typedef T V16 __attribute__((ext_vector_type(2), aligned(16)));
        P* mine = lds_piece + (size_t)wave * 16 * 4 * kPieceRow;  // idle: the last gather has read its pieces back
        wave_sync();
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          P w;
          w.x = gradv[(2 * k) % N][(2 * k) / N];
          w.y = gradv[(2 * k + 1) % N][(2 * k + 1) / N];
          mine[wl * 3 + k] = w;
        }
        wave_sync();
        V16 r[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) r[k] = *reinterpret_cast<const V16*>(mine + k * 64 + wl);
        V16* dst = reinterpret_cast<V16*>(a.grad + (p0 + wave_lp) * N);
#pragma unroll
        for (int k = 0; k < 3; ++k) stream_store(dst + k * 64 + wl, r[k]);
        wave_sync();  // the next iteration's coordinate load or gather reuses the area
        stored = true;
      }
    }
    if constexpr (kCanWide) {
      if (!stored && a.store != kPointsStoreElem && live[PPL - 1]) {
        TV* dst = reinterpret_cast<TV*>(a.grad + p0 * N);
#pragma unroll
        for (int k = 0; k < PPL * N / 2; ++k) {
          TV w;
          w.x = gradv[(2 * k) % N][(2 * k) / N];
          w.y = gradv[(2 * k + 1) % N][(2 * k + 1) / N];
          stream_store(dst + (lq * N / 2 + k), w);
        }
        stored = true;
      }
    }
    if (!stored) {  // any stride or alignment, and the batch's ragged tail
#pragma unroll
      for (int h = 0; h < PPL; ++h)
        if (live[h]) {
          T* rows = a.grad + p0 * a.gstride;
#pragma unroll
          for (int d = 0; d < N; ++d) stream_store(rows + ((lq + h) * (unsigned)a.gstride + d), gradv[d][h]);
        }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
template <typename T, int N>
struct CubicPointsGradArgs {
  const T* bricks;
  unsigned table_bytes;  // < 4 GiB
  const T* pts;
  size_t stride;
  T* out;
  T* grad;
  size_t gstride;
  unsigned long long* first_bad;
  size_t npts;
  int vec2_load;   // N == 2: stride == 2 and an aligned base: one two-element load per point
  int vec2_store;  // N == 2: gstride == 2 and an aligned base: one two-element store per point
  T start[N];
  T step[N];
  int n[N];
  AxisArgs<T, N> ax;
  unsigned plane_stride[N];  // d >= 2: table elements per unit index of dim d
  unsigned nbj;
  int linearize;
};

template <typename T, int N, bool RECT, bool FMA, int SI, int SJ>
__global__ void __launch_bounds__(kBlock) k_cubic_points_grad(const CubicPointsGradArgs<T, N> a) {
  static_assert(N == 2 || N == 3, "fused point-major multicubic gradient kernel: N = 2, 3");
  INTERPN_CUBIC_BRICK_PROLOGUE()
  typedef T TV __attribute__((ext_vector_type(2)));
  const size_t nthreads = (size_t)gridDim.x * kBlock;
  const size_t niter = (a.npts + nthreads - 1) / nthreads;
  for (size_t it = 0; it < niter; ++it) {
    // every lane runs every iteration: dead lanes take part in the gathers' exchanges with the offsets of a valid point
    const size_t i0 = it * nthreads + (size_t)blockIdx.x * kBlock + lane;
    const bool live = i0 < a.npts;
    // the point's row
    T xin[N];
#pragma unroll
    for (int d = 0; d < N; ++d) xin[d] = RECT ? (T)0 : a.start[d];
    if (live) {
      bool loaded = false;
      if constexpr (N == 2) {
        if (a.vec2_load) {
          const TV w = stream_load(reinterpret_cast<const TV*>(a.pts) + i0);
          xin[0] = w.x;
          xin[1] = w.y;
          loaded = true;
        }
      }
      if (!loaded) {
        const T* row = a.pts + i0 * a.stride;
#pragma unroll
        for (int d = 0; d < N; ++d) xin[d] = stream_load(row + d);
      }
    }
    INTERPN_CUBIC_GRAD_CELL(xin[d], live, i0)
    if (live) {
      stream_store(a.out + i0, res);
      T comp[N];
#pragma unroll
      for (int d = 0; d < N; ++d) {
        const T s = INTERPN_CUBIC_GRAD_SIGNED(d);
        comp[d] = s / width[d];
      }
      bool stored = false;
      if constexpr (N == 2) {
        if (a.vec2_store) {
          TV w;
          w.x = comp[0];
          w.y = comp[1];
          stream_store(reinterpret_cast<TV*>(a.grad) + i0, w);
          stored = true;
        }
      }
      if (!stored) {
        T* row = a.grad + i0 * a.gstride;
#pragma unroll
        for (int d = 0; d < N; ++d) stream_store(row + d, comp[d]);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
template <typename T>
struct JoinArgs {
  const T* src[kMaxDims];
  T* grad;
  size_t gstride;
  size_t count;
  int ndims;
};

// One workgroup per kBlock points: their gradient rows are kBlock * gstride consecutive elements.
template <typename T>
__global__ void __launch_bounds__(kBlock) k_join_grad(const JoinArgs<T> a) {
  __shared__ T tile[kMaxDims][kBlock + 1];
  const size_t p0 = (size_t)blockIdx.x * kBlock;
  const size_t here = a.count - p0 < (size_t)kBlock ? a.count - p0 : (size_t)kBlock;
  T* rows = a.grad + p0 * a.gstride;
  if (a.gstride > kSplitTileStride) {  // rows of long records: a lane per point, nothing to coalesce (launch-uniform)
    if (threadIdx.x < here)
      for (int d = 0; d < a.ndims; ++d) stream_store(rows + threadIdx.x * a.gstride + d, a.src[d][p0 + threadIdx.x]);
    return;
  }
  if (threadIdx.x < here)
    for (int d = 0; d < a.ndims; ++d) tile[d][threadIdx.x] = a.src[d][p0 + threadIdx.x];
  __syncthreads();
  const unsigned stride = (unsigned)a.gstride;
  const unsigned span = (unsigned)here * stride;
  for (unsigned e = threadIdx.x; e < span; e += kBlock) {
    const unsigned p = e / stride;
    const unsigned d = e - p * stride;
    // elements d >= ndims of a row are somebody else's (the last row's may not even exist): never written
    if (d < (unsigned)a.ndims) stream_store(rows + e, tile[d][p]);
  }
}

}  // namespace interpn
