// Point-major observation points: coordinate d of point i is pts[i * stride + d] (an (n, N) array, or rows of a wider
// record), evaluated without de-interleaving them first.
//
//   k_linear_points<T, N, RECT, FMA, SI, SJ, PPL, AXR, CELL>   N = 2, 3 multilinear on the re-laid table the handle already
//       has: k_linear_grad without the gradient part.  Cell search, t, the gather (3-D bricks of every layout, the 2-D
//       lane-pair gather) and the value tree are the value kernels' statements, so a result has the bits of
//       interpn_hip_eval_device on the de-interleaved columns.  Only the coordinate load is new (PointsArgs::load,
//       launch-uniform):
//         kPointsLoadElem   one element load per coordinate: any stride, any alignment
//         kPointsLoadWide   stride == N, base aligned to two elements: the lane's own PPL * N contiguous elements as
//                           two-element vector loads (3-D f64, PPL = 2: three 16-byte loads of the lane's 48 bytes)
//         kPointsLoadLds    3-D f64 with PPL = 2: the wave's 3072-byte span as three lane-contiguous 16-byte loads into the
//                           wave's own part of the piece exchange area, read back 48 bytes per lane (no LDS beyond what
//                           the gather has; waves of the ragged tail take the wide form): the automatic form there
//   k_split_points<T>   de-interleaves a slice of the block into N coordinate arrays (everything the fused kernel does not
//       take then goes through the ordinary kernels): the rows are read contiguously, each coordinate array is written
//       contiguously, through an LDS tile.
//   k_points_bad_begin / _end   one lane each, around a slice that does not start at point 0: the first-failing-index word
//       counts from the start of the whole call.
#pragma once

#include "linear_grad.h"
#include "points_forms.h"

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
  typedef typename LeafVec<T, 2>::type P;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  // N == 3: [pieces][offsets][axes] as in k_linear_brick; N == 2: the axes alone (the gather is a lane-pair swap)
  constexpr size_t kGatherLds = N == 3 ? (size_t)kBlock * kPieceRow * sizeof(P) + (size_t)kBlock * 16 : 0;
  P* lds_piece = reinterpret_cast<P*>(smem_raw);
  lds_u32* lds_off = reinterpret_cast<lds_u32*>(smem_raw + kBlock * kPieceRow * sizeof(P));
  unsigned char* lds_axes = smem_raw + kGatherLds;
  LaneAxes<T, N> la;
  if constexpr (RECT && AXR != 0) {
    la = load_lane_axes<T, N, AXR>(a.ax);
  } else if (RECT && a.ax.use_lds) {
    stage_axes<T, N>(a.ax, lds_axes);
  }
  const unsigned char* axis_base = (RECT && AXR == 0 && a.ax.use_lds) ? lds_axes : a.ax.image;
  const unsigned lane = threadIdx.x;
  const size_t nslots = (a.npts + PPL - 1) / PPL;
  const size_t first = (size_t)blockIdx.x * a.iters * kBlock;
  typedef T TV __attribute__((ext_vector_type(2)));  // naturally aligned: vector accesses of the wide form and of `out`
  constexpr bool kCanWide = (PPL * N) % 2 == 0;
  constexpr bool kCanLds = N == 3 && sizeof(T) == 8 && PPL == 2;
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
    bool loaded = false;
    if constexpr (kCanLds) {
      const unsigned wl = lane & 63u;
      const size_t wave_p0 = (s0 - wl) * PPL;  // the wave's first point; it has 64 * PPL of them
      if (a.load == kPointsLoadLds && wave_p0 + 64 * PPL <= a.npts) {  // wave-uniform
        typedef T V16 __attribute__((ext_vector_type(2), aligned(16)));
        // the wave's quads' rows of the piece area: 16 quads x 4 rows x kPieceRow slots, idle until the gather
        P* mine = lds_piece + (size_t)(lane >> 6) * 16 * 4 * kPieceRow;
        static_assert(16 * 4 * kPieceRow >= 64 * PPL * N / 2, "a wave's span fits its part of the piece area");
        const V16* src = reinterpret_cast<const V16*>(a.pts + wave_p0 * N);
        V16 r[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) r[k] = stream_load(src + k * 64 + wl);
#pragma unroll
        for (int k = 0; k < 3; ++k) *reinterpret_cast<V16*>(mine + k * 64 + wl) = r[k];
        wave_sync();
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const P w = mine[wl * 3 + k];
          xin[(2 * k) / N][(2 * k) % N] = w.x;
          xin[(2 * k + 1) / N][(2 * k + 1) % N] = w.y;
        }
        wave_sync();
        loaded = true;
      }
    }
    if constexpr (kCanWide) {
      if (!loaded && a.load != kPointsLoadElem && live[PPL - 1]) {
        const TV* src = reinterpret_cast<const TV*>(a.pts + i0 * N);
#pragma unroll
        for (int k = 0; k < PPL * N / 2; ++k) {
          const TV w = stream_load(src + k);
          xin[(2 * k) / N][(2 * k) % N] = w.x;
          xin[(2 * k + 1) / N][(2 * k + 1) % N] = w.y;
        }
        loaded = true;
      }
    }
    if (!loaded) {  // any stride or alignment, and the batch's ragged tail
#pragma unroll
      for (int h = 0; h < PPL; ++h)
        if (live[h]) {
          const T* row = a.pts + (i0 + h) * a.stride;
#pragma unroll
          for (int d = 0; d < N; ++d) xin[h][d] = stream_load(row + d);
        }
    }
    int cell_r[PPL][N];
    T x0_r[PPL][N], x1_r[PPL][N];
    if constexpr (RECT && AXR != 0) lane_axes_locate<T, N, PPL, AXR>(a.ax, la, xin, cell_r, x0_r, x1_r);
    T resv[PPL];
#pragma unroll
    for (int h = 0; h < PPL; ++h) {
      T t[N];
      int loc[N];
      bool ok = true;
#pragma unroll
      for (int d = 0; d < N; ++d) {
        const T x = xin[h][d];
        if (RECT) {
          T x0, x1;
          int l;
          if constexpr (AXR != 0) {
            l = cell_r[h][d];
            x0 = x0_r[h][d];
            x1 = x1_r[h][d];
          } else {
            const Axis<T> ax = make_axis<T, N>(a.ax, axis_base, d);
            l = axis_cell<T>(ax, x, &x0, &x1);  // multilinear/rectilinear.rs:353-370, :310-311
          }
          const T step = x1 - x0;
          t[d] = (x - x0) / step;  // rectilinear.rs:310-313
          loc[d] = l;
        } else {
          T floc;
          ok &= regular_floc<T>(x, a.start[d], a.step[d], &floc);  // multilinear/regular.rs:415-418
          const int l = clamp_loc<T>(floc, a.n[d] - 2);             // regular.rs:420-422
          const T izl = mul_add<FMA>(a.step[d], (T)l, a.start[d]);  // regular.rs:334-337
          t[d] = (x - izl) / a.step[d];                             // regular.rs:339
          loc[d] = l;
        }
      }
      if (!RECT && !ok && live[h]) atomicMin(a.first_bad, (unsigned long long)(i0 + h));
      if constexpr (N == 3) {
        typedef BrickGeom<T, CELL> Geom;
        const unsigned q = lane & 3;
        const unsigned quad = lane >> 2;
        const unsigned bk = (unsigned)loc[2] / (unsigned)Geom::SK;
        const unsigned kpart = bk * (unsigned)Geom::ELEMS + ((unsigned)loc[2] - bk * (unsigned)Geom::SK);
#pragma unroll
        for (int p = 0; p < 4; ++p)
          lds_off[(quad * 4 + p) * 4 + q] = brick_piece<T, SI, SJ, CELL>(a.nbj, a.nbk, loc[0], loc[1], kpart, p >> 1, p & 1);
        wave_sync();
        const uint4 toff = *reinterpret_cast<const uint4*>(&lds_off[(quad * 4 + q) * 4]);
        const Cell<T> c = gather_cell<T>(a.bricks, toff, 0u, lds_piece, quad, q);
        // the tree of k_linear_brick (i first, k last; multilinear/regular.rs:347-403)
        T r[2];
#pragma unroll
        for (int dk = 0; dk < 2; ++dk) {
          const T c0 = grad_lerp<FMA>(t[0], c.v[0][0][dk], c.v[1][0][dk]);
          const T c1 = grad_lerp<FMA>(t[0], c.v[0][1][dk], c.v[1][1][dk]);
          r[dk] = grad_lerp<FMA>(t[1], c0, c1);
        }
        resv[h] = grad_lerp<FMA>(t[2], r[0], r[1]);
      } else {
        // the lane-pair gather of k_linear2_brick: brick (bi = i, bj = j / SJ2), two row pieces per point
        constexpr unsigned KW2 = 64 / sizeof(T), SJ2 = KW2 - 1, EL2 = 2 * KW2;
        const unsigned q = lane & 1;
        const unsigned bj = (unsigned)loc[1] / SJ2;
        const unsigned mine = ((unsigned)loc[0] * a.nbj + bj) * EL2 + ((unsigned)loc[1] - bj * SJ2);
        const unsigned theirs = grad_swap1(mine);
        const unsigned off0 = (q == 0 ? mine : theirs) + q * KW2;
        const unsigned off1 = (q == 0 ? theirs : mine) + q * KW2;
        const P p0 = *reinterpret_cast<const P*>(a.bricks + off0);
        const P p1 = *reinterpret_cast<const P*>(a.bricks + off1);
        const P keep = q == 0 ? p0 : p1;
        const P send = q == 0 ? p1 : p0;
        P recv;
        recv.x = grad_swap1(send.x);
        recv.y = grad_swap1(send.y);
        const P row0 = q == 0 ? keep : recv;  // v(i, j), v(i, j+1)
        const P row1 = q == 0 ? recv : keep;  // row i+1
        const T c0 = grad_lerp<FMA>(t[0], row0.x, row1.x);
        const T c1 = grad_lerp<FMA>(t[0], row0.y, row1.y);
        resv[h] = grad_lerp<FMA>(t[1], c0, c1);
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
