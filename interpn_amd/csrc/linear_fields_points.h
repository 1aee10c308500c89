// Point-major field sets: the points as one (n, N) array, the results as one (n, K) array, one pass
// (include/interpn_hip.h, "Point-major field sets").
//
//   k_linear_fields_points<T, N, RECT, FMA>   N = 2, 3 on the fused table a set already has (linear_fields.h).  Everything
//       between the coordinate load and the result store is INTERPN_FIELDS_LOCATE / INTERPN_FIELDS_GROUP of linear_fields.h,
//       the statements of k_linear_fields, so field f of point i has the bits of row f of that kernel.
//       Coordinate load (FieldsPointsArgs::load, launch-uniform, chosen on the host):
//         kPointsLoadLds    stride == N: the wave's 64 * N contiguous elements as N lane-contiguous element loads into the
//                           wave's s_t area (idle until the cell search has run), read back N per lane.  Element loads, so
//                           any element-aligned base will do; a ragged last wave loads the elements that exist.
//         kPointsLoadElem   any stride: N element loads per lane from the point's own row.
//       Elements d >= N of a row are never read, lanes behind the batch read nothing.
//       Result store: the wave stages a [64][KT] tile in LDS (rows TS = KT + 1 elements apart: the tree's lanes write
//       a column of it, 8 rows per instruction, and an odd row pitch keeps them on different banks), KT = 8 = the largest
//       P, so a tile is KT / P whole line groups.  The tile's 64 * Kw elements (Kw = the tile's fields, K or KT or the
//       last tile's rest) are then stored lane-contiguously: element e of the tile is field f0 + e % Kw of point e / Kw,
//       at out[(wbase + e / Kw) * out_stride + f0 + e % Kw].  With out_stride == K <= KT that is one contiguous run of
//       64 * K elements per wave; otherwise runs of Kw elements per row.  Elements f >= K of a row are never written.
//   k_join_fields<T>   the split path's last step: (K, count) rows of scratch into the caller's (count, K) rows, through an
//       LDS tile of kJoinTile fields x kBlock points; any K (a loop over tiles), runs of min(K - f0, kJoinTile) elements
//       per row, nothing written at f >= K.
#pragma once

#include "linear_fields.h"
#include "points_forms.h"

namespace interpn {

template <typename T, int N>
struct FieldsPointsLayout {
  static constexpr int KT = 8;       // fields of a tile: a multiple of every P (2, 4, 8)
  static constexpr int TS = KT + 1;  // elements from row to row of the tile
  // LDS of one wave: first line of the cell (u32) and t[N] of its 64 points (the coordinate load's landing area before
  // that), then the result tile
  static constexpr unsigned kWaveLds = 64u * 4u + (unsigned)(N * 64 + 64 * TS) * (unsigned)sizeof(T);
  static_assert(KT % FieldsLayout<T, N>::P == 0, "a tile is whole line groups");
};

template <typename T, int N>
struct FieldsPointsArgs {
  const unsigned char* table;
  const T* pts;
  size_t stride;      // elements from point to point, >= N
  T* out;
  size_t out_stride;  // elements from point to point, >= nfields
  unsigned long long* first_bad;
  size_t npts;
  int nfields;
  int load;             // PointsLoad: kPointsLoadLds (stride == N) or kPointsLoadElem
  unsigned groups;      // lines per cell: ceil(nfields / P)
  unsigned cstride[N];  // lines between neighbouring cells along each dimension (C order, times `groups`)
  T start[N];
  T step[N];
  int n[N];
  AxisArgs<T, N> ax;    // rectilinear grids only
};

template <typename T, int N, bool RECT, bool FMA>
__global__ void __launch_bounds__(kBlock) k_linear_fields_points(const FieldsPointsArgs<T, N> a) {
  typedef FieldsLayout<T, N> L;
  typedef FieldsPointsLayout<T, N> PL;
  typedef T V __attribute__((ext_vector_type(L::EPP)));
  INTERPN_FIELDS_PROLOGUE(PL::kWaveLds);
  T* s_tile = s_t + N * 64;
  constexpr unsigned kTileGroups = PL::KT / L::P;

  // whole workgroups iterate together, as in k_linear_fields: every lane of a wave stays active
  for (size_t base = (size_t)blockIdx.x * kBlock; base < a.npts; base += (size_t)gridDim.x * kBlock) {
    const size_t i = base + threadIdx.x;
    const bool live = i < a.npts;
    const size_t wbase = base + (size_t)wave * 64;
    const unsigned here = wbase >= a.npts ? 0u : (a.npts - wbase < 64 ? (unsigned)(a.npts - wbase) : 64u);  // the wave's points
    T xin[N];
#pragma unroll
    for (int d = 0; d < N; ++d) xin[d] = RECT ? (T)0 : a.start[d];
    if (a.load == kPointsLoadLds) {  // launch-uniform
      const T* span = a.pts + wbase * N;
#pragma unroll
      for (int k = 0; k < N; ++k) {
        const unsigned e = (unsigned)k * 64u + (unsigned)lane;
        if (e < here * N) s_t[e] = stream_load(span + e);
      }
      wave_sync();
      if (live) {
#pragma unroll
        for (int d = 0; d < N; ++d) xin[d] = s_t[lane * N + d];
      }
      wave_sync();
    } else if (live) {
      const T* row = a.pts + i * a.stride;
#pragma unroll
      for (int d = 0; d < N; ++d) xin[d] = stream_load(row + d);
    }
    INTERPN_FIELDS_LOCATE(xin[d], live, i);
    for (unsigned g0 = 0; g0 < a.groups; g0 += kTileGroups) {
      const unsigned gend = a.groups - g0 < kTileGroups ? a.groups : g0 + kTileGroups;
      for (unsigned g = g0; g < gend; ++g) {
        INTERPN_FIELDS_GROUP(g, s_tile[p * PL::TS + (int)(g - g0) * L::P + fl]);
      }
      wave_sync();
      // the tile's fields [f0, f0 + kw) of the wave's `here` points, lane-contiguously
      const unsigned f0 = g0 * (unsigned)L::P;
      const unsigned left = (unsigned)a.nfields - f0;
      const unsigned kw = left < (unsigned)PL::KT ? left : (unsigned)PL::KT;
      const unsigned q = 64u / kw, r = 64u - q * kw;  // uniform: what 64 more elements add to (point, field)
      unsigned p = (unsigned)lane / kw;
      unsigned f = (unsigned)lane - p * kw;
      T* dst = a.out + wbase * a.out_stride + f0;
      for (unsigned k = 0; k < kw; ++k) {
        if (p < here) stream_store(dst + (size_t)p * a.out_stride + f, s_tile[p * PL::TS + f]);
        p += q;
        f += r;
        if (f >= kw) {
          f -= kw;
          ++p;
        }
      }
      wave_sync();
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
constexpr int kJoinTile = 8;  // fields of k_join_fields' LDS tile

template <typename T>
struct JoinFieldsArgs {
  const T* src;       // row f at src + f * pitch
  size_t pitch;       // elements
  T* out;
  size_t out_stride;  // elements from point to point, >= nfields
  size_t count;
  size_t nfields;
};

// One workgroup per kBlock points.
template <typename T>
__global__ void __launch_bounds__(kBlock) k_join_fields(const JoinFieldsArgs<T> a) {
  __shared__ T tile[kJoinTile][kBlock + 1];
  const size_t p0 = (size_t)blockIdx.x * kBlock;
  const unsigned here = a.count - p0 < (size_t)kBlock ? (unsigned)(a.count - p0) : (unsigned)kBlock;
  T* rows = a.out + p0 * a.out_stride;
  for (size_t f0 = 0; f0 < a.nfields; f0 += kJoinTile) {
    const unsigned kw = a.nfields - f0 < (size_t)kJoinTile ? (unsigned)(a.nfields - f0) : (unsigned)kJoinTile;
    if (threadIdx.x < here)
      for (unsigned f = 0; f < kw; ++f) tile[f][threadIdx.x] = stream_load(a.src + (f0 + f) * a.pitch + p0 + threadIdx.x);
    __syncthreads();
    const unsigned span = here * kw;
    for (unsigned e = threadIdx.x; e < span; e += kBlock) {
      const unsigned p = e / kw;
      const unsigned f = e - p * kw;
      stream_store(rows + (size_t)p * a.out_stride + f0 + f, tile[f][p]);
    }
    __syncthreads();
  }
}

}  // namespace interpn
