// Gradients of a field set: K values and their K x N Jacobian in one pass over the points (include/interpn_hip.h,
// "Gradients of a field set").  N = 2, 3; regular and rectilinear; f64 and f32; any K; on the set's fused table
// (linear_fields.h) — no table of its own, and no table line beyond those of a value call.
//
// Definition.  Row f of `out` has the bits of k_linear_fields; component d of field f has the bits of the single handle's
// gradient (linear_grad.h, DESIGN.md "Gradients"):
//   W[c']   = V[c' | 1 << d] - V[c']           one subtraction per corner pair
//   s       = W reduced over e != d, ascending e, with fields_node(t[e], y0, y1)
//   grad[d] = s / h[d]                          IEEE division; h = step[d], or x1 - x0 of the point's cell
//
// Kernel.  Prologue, cell search and line-group walk are k_linear_fields': a lane locates its point, the wave shares
// {first line of the cell, t[N]} through LDS, 8 lanes x 16 bytes fetch one point's line of a group.  Over the piece of a
// point a lane then reduces N + 1 trees per field — the value, then the components in ascending d:
//   d inside a piece (dim 0 in f64; dims 0, 1 in f32)   the W pairs are differences of the lane's own elements; the other
//       in-piece dimension (f32), then the cross-lane dimensions in ascending order.
//   d across lanes (partner = lane ^ 1 or lane ^ 2)      the partner's piece comes through the quad permute FIRST, both
//       lanes of the pair form the same W = upper - lower element by element, then the in-piece levels, then the other
//       cross-lane dimension.
// The results go to P (N + 1) rows of 64 in LDS (FieldsGradLayout::kWaveLds), and lane l stores element l of every row:
// one contiguous 64-element run per row and wave.  Lane l is also the lane that located point l, so the cell width of the
// point it stores is in its own registers: the ONE division of a component happens there, once per stored element, and
// the widths never travel through LDS.  Padding fields of the last line are reduced and never stored.
#pragma once

#include "linear_fields.h"

namespace interpn {

template <typename T, int N>
struct FieldsGradArgs {
  const unsigned char* table;
  const T* obs[N];
  T* out;
  size_t out_stride;   // elements between the value rows of two fields
  T* grad;
  size_t grad_stride;  // elements between two of the K * N component rows: row (f * N + d)
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

// INTERPN_FIELDS_LOCATE with the cell's width kept: declares width[N] beside t[N] (rectilinear: the `step` that t was
// divided by; regular: a.step[d]).  Everything else is that macro's text (linear_fields.h), which stays as it is for
// k_linear_fields and k_linear_fields_points.
#define INTERPN_FIELDS_GRAD_LOCATE(X, LIVE, INDEX) \
  T t[N], width[N];                                                                                              \
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
      width[d] = step;                                                                                           \
    } else {                                                                                                     \
      const T x = (X);                                                                                           \
      T floc;                                                                                                    \
      ok &= regular_floc<T>(x, a.start[d], a.step[d], &floc);  /* regular.rs:415-418 */                          \
      loc = clamp_loc<T>(floc, a.n[d] - 2);                    /* regular.rs:420-422 */                          \
      const T index_zero_loc = mul_add<FMA>(a.step[d], (T)loc, a.start[d]);  /* regular.rs:334-339 */            \
      t[d] = (x - index_zero_loc) / a.step[d];                                                                   \
      width[d] = a.step[d];                                                                                      \
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

// INTERPN_FIELDS_GRAD_FETCH(G)  declares v[8]: this lane's piece of line group G for the 8 points it serves (the loads
//     of INTERPN_FIELDS_GROUP).
#define INTERPN_FIELDS_GRAD_FETCH(G) \
  V v[8];                                                                                                                 \
  _Pragma("unroll")                                                                                                       \
  for (int j = 0; j < 8; ++j)                                                                                             \
    v[j] = *reinterpret_cast<const V*>(a.table + ((size_t)lines[j] + (G)) * L::kLineBytes + (unsigned)piece * 16u);

// INTERPN_FIELDS_GRAD_TREE(C, PV, R)  R = the tree of round C over the piece PV with the point's tt[N]: C = -1 the value
//     (INTERPN_FIELDS_GROUP's tree), C = d >= 0 the undivided component d.  Every lane of a field's 2^XB lanes ends with R.
#define INTERPN_FIELDS_GRAD_TREE(C, PV, R) \
  if constexpr ((C) < 0) {                                                                                                \
    if constexpr (L::LB == 1) {                                                                                           \
      R = fields_node<FMA, T>(tt[0], (PV)[0], (PV)[1]);                                                                   \
    } else {                                                                                                              \
      const T r0 = fields_node<FMA, T>(tt[0], (PV)[0], (PV)[1]);                                                          \
      const T r1 = fields_node<FMA, T>(tt[0], (PV)[2], (PV)[3]);                                                          \
      R = fields_node<FMA, T>(tt[1], r0, r1);                                                                             \
    }                                                                                                                     \
    if constexpr (L::XB >= 1) R = fields_cross_level<0, FMA, T>(R, tt[L::LB], piece);                                     \
    if constexpr (L::XB >= 2) R = fields_cross_level<1, FMA, T>(R, tt[L::LB + 1], piece);                                 \
  } else if constexpr ((C) < L::LB) {                                                                                     \
    /* d inside the piece: the W pairs are local */                                                                      \
    if constexpr (L::LB == 1) {                                                                                           \
      R = (PV)[1] - (PV)[0];                                                                                              \
    } else if constexpr ((C) == 0) {                                                                                      \
      R = fields_node<FMA, T>(tt[1], (PV)[1] - (PV)[0], (PV)[3] - (PV)[2]);                                               \
    } else {                                                                                                              \
      R = fields_node<FMA, T>(tt[0], (PV)[2] - (PV)[0], (PV)[3] - (PV)[1]);                                               \
    }                                                                                                                     \
    if constexpr (L::XB >= 1) R = fields_cross_level<0, FMA, T>(R, tt[L::LB], piece);                                     \
    if constexpr (L::XB >= 2) R = fields_cross_level<1, FMA, T>(R, tt[L::LB + 1], piece);                                 \
  } else {                                                                                                                \
    /* d across lanes: the partner's piece first, the same W in both lanes of the pair */                                 \
    constexpr int kx = ((C) - L::LB) & 1;                                                                                 \
    const bool upper = ((piece >> kx) & 1) != 0;                                                                          \
    T w[L::EPP];                                                                                                          \
    _Pragma("unroll")                                                                                                     \
    for (int e = 0; e < L::EPP; ++e) {                                                                                    \
      const T mine = (PV)[e];                                                                                             \
      const T other = quad_xor<(1 << kx)>(mine);                                                                          \
      w[e] = (upper ? mine : other) - (upper ? other : mine);                                                             \
    }                                                                                                                     \
    if constexpr (L::LB == 1) {                                                                                           \
      R = fields_node<FMA, T>(tt[0], w[0], w[1]);                                                                         \
    } else {                                                                                                              \
      const T r0 = fields_node<FMA, T>(tt[0], w[0], w[1]);                                                                \
      const T r1 = fields_node<FMA, T>(tt[0], w[L::EPP - 2], w[L::EPP - 1]);                                              \
      R = fields_node<FMA, T>(tt[1], r0, r1);                                                                             \
    }                                                                                                                     \
    if constexpr (L::XB >= 2) R = fields_cross_level<1 - kx, FMA, T>(R, tt[L::LB + 1 - kx], piece);                       \
  }

// INTERPN_FIELDS_GRAD_STAGE(C)  inside the loop over the lane's 8 points: the tree of C over v[j] into row (C + 1) * P + fl
//     of s_res, at the point's place p.
#define INTERPN_FIELDS_GRAD_STAGE(C) \
  {                                                                                                                       \
    T r;                                                                                                                  \
    INTERPN_FIELDS_GRAD_TREE(C, v[j], r)                                                                                  \
    if (owner) s_res[(((C) + 1) * L::P + fl) * 64 + p] = r;                                                               \
  }

// INTERPN_FIELDS_GRAD_STORE(C, ROW0, RSTRIDE)  element `lane` of the P rows of C to ROW0 + fl * RSTRIDE (ROW0: the row of
//     the group's first field; RSTRIDE: elements between the rows of two fields), divided by this lane's width[C] on the
//     way when C is a component.  Fields beyond K — the padding of the last line — are not stored.
#define INTERPN_FIELDS_GRAD_STORE(C, ROW0, RSTRIDE) \
  _Pragma("unroll")                                                                                                       \
  for (int fl = 0; fl < L::P; ++fl) {                                                                                     \
    T res = s_res[(((C) + 1) * L::P + fl) * 64 + lane];                                                                   \
    if constexpr ((C) >= 0) res = res / width[(C) < 0 ? 0 : (C)];                                                         \
    if (f0 + fl < (size_t)a.nfields && store_live) stream_store((ROW0) + (size_t)fl * (RSTRIDE) + wbase + lane, res);     \
  }

template <typename T, int N>
struct FieldsGradLayout {
  typedef FieldsLayout<T, N> L;
  // LDS of one wave: first line of the cell (u32) and t[N] of its 64 points, then P result rows for the value and for
  // each of the N components
  static constexpr unsigned kWaveLds = 64u * 4u + (unsigned)(N + L::P * (N + 1)) * 64u * (unsigned)sizeof(T);
};

template <typename T, int N, bool RECT, bool FMA>
__global__ void __launch_bounds__(kBlock) k_linear_fields_grad(const FieldsGradArgs<T, N> a) {
  typedef FieldsLayout<T, N> L;
  typedef T V __attribute__((ext_vector_type(L::EPP)));
  INTERPN_FIELDS_PROLOGUE((FieldsGradLayout<T, N>::kWaveLds));
  T* s_res = s_t + N * 64;

  // whole workgroups iterate together: every lane of a wave stays active (the exchanges below need it);
  // lanes behind the batch evaluate a harmless coordinate and only their stores are masked
  for (size_t base = (size_t)blockIdx.x * kBlock; base < a.npts; base += (size_t)gridDim.x * kBlock) {
    const size_t i = base + threadIdx.x;
    const bool live = i < a.npts;
    INTERPN_FIELDS_GRAD_LOCATE(live ? stream_load(a.obs[d] + i) : (RECT ? (T)0 : a.start[d]), live, i);
    const size_t wbase = base + (size_t)__builtin_amdgcn_readfirstlane(wave) * 64;  // wave-uniform: the row addresses stay scalar
    const bool store_live = wbase + lane < a.npts;
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
        INTERPN_FIELDS_GRAD_STAGE(-1);
        INTERPN_FIELDS_GRAD_STAGE(0);
        INTERPN_FIELDS_GRAD_STAGE(1);
        if constexpr (N == 3) INTERPN_FIELDS_GRAD_STAGE(2);
      }
      wave_sync();
      const size_t f0 = (size_t)g * L::P;
      T* const grow = a.grad + f0 * N * a.grad_stride;  // component row 0 of field f0; N rows on: field f0 + 1
      INTERPN_FIELDS_GRAD_STORE(-1, a.out + f0 * a.out_stride, a.out_stride);
      INTERPN_FIELDS_GRAD_STORE(0, grow, (size_t)N * a.grad_stride);
      INTERPN_FIELDS_GRAD_STORE(1, grow + a.grad_stride, (size_t)N * a.grad_stride);
      if constexpr (N == 3) { INTERPN_FIELDS_GRAD_STORE(2, grow + 2 * a.grad_stride, (size_t)N * a.grad_stride); }
      wave_sync();
    }
  }
}

}  // namespace interpn
