// Point-major gradients of a field set: the points as one (n, N) array, the K values as one (n, K) array and the Jacobian
// as one (n, K, N) array, one pass (include/interpn_hip.h, "Point-major gradients of a field set").  N = 2, 3; regular and
// rectilinear; f64 and f32; any K; on the set's fused table (linear_fields.h) — no table of its own, and no table line
// beyond those of a value call.
//
// Definition, by reference: out[i * out_stride + f] has the bits of k_linear_fields_points (those of k_linear_fields on the
// columns), jac[i * jac_stride + f * N + d] the bits of row f * N + d of k_linear_fields_grad on the columns.
//
//   k_linear_fields_points_grad<T, N, RECT, FMA>
//       Between the coordinate load and the stores nothing is new: INTERPN_FIELDS_PROLOGUE (linear_fields.h), the coordinate
//       load of k_linear_fields_points in both forms (kPointsLoadLds / kPointsLoadElem, linear_fields_points.h),
//       INTERPN_FIELDS_GRAD_LOCATE, INTERPN_FIELDS_GRAD_FETCH and INTERPN_FIELDS_GRAD_TREE (linear_fields_grad.h): the value
//       tree first, then the components in ascending d.  Those headers stay as they are; what is new stands here.
//       Staging (point-major, FieldsPointsGradLayout): per line group a point owns a row of P * N undivided components
//       (element fl * N + d, rows JS = P * N + 1 elements apart) and a row of P values (rows VS = P + 1 apart).  P * N and P
//       are even, so both pitches are odd: the 8 points whose trees end in one instruction land on different banks, and
//       the store's lane-contiguous read walks the rows in address order (one skipped element per point).
//       The one division: the cell width of a rectilinear point lives in the lane that located it, which is not the lane
//       that stores its components.  width[N] therefore travels through LDS next to t[N] (s_w, rectilinear only; a regular
//       grid divides by the launch-uniform a.step[d]), and the storing lane divides the undivided tree result it read by
//       s_w[d * 64 + p]: the operands, and so the bits, of k_linear_fields_grad's division.
//       Stores: per group the run of a point is kw * N Jacobian elements and kw values, kw = min(P, K - f0).  Element e of
//       the wave's 64 * run elements is offset e % run of point e / run, at jac[(wbase + e / run) * jac_stride + f0 * N +
//       e % run] (values alike): with jac_stride == K * N and one line group one contiguous run of 64 K N elements per
//       wave.  Row addresses are size_t.  Nothing is written beyond K (values) or K * N (components) of a row; the padding
//       fields of the last line are staged and never read back.
#pragma once

#include "linear_fields_grad.h"
#include "linear_fields_points.h"

namespace interpn {

template <typename T, int N, bool RECT>
struct FieldsPointsGradLayout {
  typedef FieldsLayout<T, N> L;
  static constexpr int JS = L::P * N + 1;  // elements from point to point of the component tile (odd)
  static constexpr int VS = L::P + 1;      // ... of the value tile (odd)
  static constexpr int kWidths = RECT ? N : 0;  // width[N] rows beside t[N]
  // LDS of one wave: first line of the cell (u32), t[N] of its 64 points (the coordinate load's landing area before that),
  // width[N] (rectilinear), then the two tiles
  static constexpr unsigned kWaveLds = 64u * 4u + (unsigned)((N + kWidths) * 64 + 64 * (JS + VS)) * (unsigned)sizeof(T);
};

template <typename T, int N>
struct FieldsPointsGradArgs {
  const unsigned char* table;
  const T* pts;
  size_t stride;      // elements from point to point, >= N
  T* out;
  size_t out_stride;  // elements from point to point, >= nfields
  T* jac;
  size_t jac_stride;  // elements from point to point, >= nfields * N
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

// INTERPN_FIELDS_POINTS_GRAD_STAGE(C)  inside the loop over the lane's 8 points: the tree of C over v[j] to the point's row
//     of the value tile (C = -1) or of the component tile (C = d), at the field's place.
#define INTERPN_FIELDS_POINTS_GRAD_STAGE(C) \
  {                                                                                                                       \
    T r;                                                                                                                  \
    INTERPN_FIELDS_GRAD_TREE(C, v[j], r)                                                                                  \
    if (owner) {                                                                                                          \
      if constexpr ((C) < 0) s_val[p * PL::VS + fl] = r;                                                                  \
      else s_jac[p * PL::JS + fl * N + ((C) < 0 ? 0 : (C))] = r;                                                          \
    }                                                                                                                     \
  }

template <typename T, int N, bool RECT, bool FMA>
__global__ void __launch_bounds__(kBlock) k_linear_fields_points_grad(const FieldsPointsGradArgs<T, N> a) {
  typedef FieldsLayout<T, N> L;
  typedef FieldsPointsGradLayout<T, N, RECT> PL;
  typedef T V __attribute__((ext_vector_type(L::EPP)));
  INTERPN_FIELDS_PROLOGUE(PL::kWaveLds);
  T* s_w = s_t + N * 64;
  T* s_jac = s_w + PL::kWidths * 64;
  T* s_val = s_jac + 64 * PL::JS;

  // whole workgroups iterate together, as in k_linear_fields_grad: every lane of a wave stays active (the exchanges below
  // need it); lanes behind the batch locate a harmless coordinate and only their stores are masked
  for (size_t base = (size_t)blockIdx.x * kBlock; base < a.npts; base += (size_t)gridDim.x * kBlock) {
    const size_t i = base + threadIdx.x;
    const bool live = i < a.npts;
    const size_t wbase = base + (size_t)__builtin_amdgcn_readfirstlane(wave) * 64;  // wave-uniform: the row addresses stay scalar
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
    INTERPN_FIELDS_GRAD_LOCATE(xin[d], live, i);
    (void)width;  // (regular grids divide by a.step[d])
    if constexpr (RECT) {
      // the widths of this lane's cell, for the lanes that will store its components (read behind the next wave_sync)
#pragma unroll
      for (int d = 0; d < N; ++d) s_w[d * 64 + lane] = width[d];
    }
    const int fl = piece >> L::XB;                               // the field of the line this lane's piece belongs to
    const bool owner = (piece & ((1 << L::XB) - 1)) == 0;        // ... and whether this lane stages its results
    for (unsigned g = 0; g < a.groups; ++g) {
      INTERPN_FIELDS_GRAD_FETCH(g);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int p = j * 8 + psub;
        T tt[N];
#pragma unroll
        for (int d = 0; d < N; ++d) tt[d] = s_t[d * 64 + p];
        INTERPN_FIELDS_POINTS_GRAD_STAGE(-1);
        INTERPN_FIELDS_POINTS_GRAD_STAGE(0);
        INTERPN_FIELDS_POINTS_GRAD_STAGE(1);
        if constexpr (N == 3) INTERPN_FIELDS_POINTS_GRAD_STAGE(2);
      }
      wave_sync();
      // the group's fields [f0, f0 + kw) of the wave's `here` points, lane-contiguously: values, then components
      const unsigned f0 = g * (unsigned)L::P;
      const unsigned left = (unsigned)a.nfields - f0;
      const unsigned kw = left < (unsigned)L::P ? left : (unsigned)L::P;
      {
        const unsigned q = 64u / kw, r = 64u - q * kw;  // uniform: what 64 more elements add to (point, field)
        unsigned p = (unsigned)lane / kw;
        unsigned f = (unsigned)lane - p * kw;
        T* dst = a.out + wbase * a.out_stride + f0;
        for (unsigned k = 0; k < kw; ++k) {
          if (p < here) stream_store(dst + (size_t)p * a.out_stride + f, s_val[p * PL::VS + f]);
          p += q;
          f += r;
          if (f >= kw) {
            f -= kw;
            ++p;
          }
        }
      }
      {
        const unsigned run = kw * (unsigned)N;
        const unsigned q = 64u / run, r = 64u - q * run;  // uniform: what 64 more elements add to (point, offset)
        unsigned p = (unsigned)lane / run;
        unsigned off = (unsigned)lane - p * run;
        T* dst = a.jac + wbase * a.jac_stride + (size_t)f0 * N;
        for (unsigned k = 0; k < run; ++k) {
          if (p < here) {
            const unsigned d = off % (unsigned)N;
            T h;
            if constexpr (RECT) {
              h = s_w[d * 64u + p];
            } else {
              h = a.step[0];
              if (d == 1u) h = a.step[1];
              if constexpr (N == 3) {
                if (d == 2u) h = a.step[2];
              }
            }
            const T res = s_jac[p * PL::JS + off] / h;  // the ONE division of a component (linear_fields_grad.h)
            stream_store(dst + (size_t)p * a.jac_stride + off, res);
          }
          p += q;
          off += r;
          if (off >= run) {
            off -= run;
            ++p;
          }
        }
      }
      wave_sync();
    }
  }
}

}  // namespace interpn
