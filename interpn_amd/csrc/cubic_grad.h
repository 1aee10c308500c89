// Multicubic value AND gradient (d/dx of every point) in one pass.
//
// The definition (DESIGN.md "Multicubic gradients") in one paragraph: per dimension the value path's footprint origin,
// saturation class, linearized flag and local coordinate tt; the value tree reduces dimension 0 first and N - 1 last with
// the 1-D node I_e; the DERIVATIVE NODE D_e works on the same four inputs from the c1, c2, c3 (Hermite arms) or k1
// (linearized arms) that I_e computes:
//   Hermite arms     e2 = c2 + c2, e3 = 3 c3, s = (e3 tt + e2) tt + c1   (fused like the value's Horner steps, or not)
//   linearized arms  s = k1
// Component d: levels e < d are the value's own partial results; level d applies D_d; levels e > d apply I_e;
// grad[d] = (Low class along d ? -s : s) / h_d with ONE division (h_d = steps[d], or the spacing the arm's t was
// divided by on a rectilinear grid).
//
//   k_cubic_grad<T, N, RECT, FMA, SI, SJ>   N = 2, 3 on the tiled table a cubic handle already has (cubic_brick.h): the
//       coordinate load, the locate step, both gathers (the 16-lane transpose and, for steps 1,1, LDS-DMA) and the plane
//       order are k_cubic_brick's; where that kernel carries one partial result per level this one carries the value and
//       one partial per component d <= level.  No binned / gated forms, no per-cell records, no interior-wave or packed-f32
//       shortcuts; rectilinear nodes divide as the reference writes them (cubic_rect_node's divisions: the fast form with
//       its whole-wave second evaluation would double the 12 live partials of a 3-D f64 point for a path that pays for
//       sorted points, which a gradient call does not have).  The kernel is its coordinate load, the gradient cell of
//       cubic_cell.h (INTERPN_CUBIC_BRICK_PROLOGUE, INTERPN_CUBIC_GRAD_CELL: shared with k_cubic_points_grad, points_grad.h)
//       on the nodes and gathers below, and its stores.
//   k_cubic_grad_n<T, KIND, FMA>   runtime N = 1..8 on the C-ordered grid: the locate step (INTERPN_CUBIC_CLASS) and value
//       walk of k_generic, then one walk per component with D at level d.  Written for correctness, not tuned.
#pragma once

#include "cubic_brick.h"

namespace interpn {

// The derivative of the Hermite arm's polynomial in tt, from the coefficients the value node computed.
template <bool FMA, typename T>
__device__ __forceinline__ T hermite_deriv(T t, T c1, T c2, T c3) {
  const T one = (T)1;
  const T three = (one + one) + one;
  const T e2 = c2 + c2;
  const T e3 = three * c3;
  if constexpr (FMA) {
    return dev_fma<T>(dev_fma<T>(e3, t, e2), t, c1);
  } else {
    T i0 = t * e3;
    T i1 = e2 + i0;
    T i2 = t * i1;
    return c1 + i2;
  }
}

// I and D of one node, regular grid: cubic_regular_node's operations (value bits are that function's), the derivative
// node on the same c1, c2, c3 / k1.
template <bool FMA, typename T, bool ARMS = false>
__device__ __forceinline__ void cubic_regular_node_vd(T v0, T v1, T v2, T v3, const CubicDimRegular<T>& d, T& val, T& der) {
  const T two = (T)2, one = (T)1;
  const bool low = d.sat == kSatLow;
  const bool high = d.sat == kSatHigh;
  T y0 = high ? v2 : v1;
  T ya = low ? v0 : (high ? v3 : v2);
  T dy = ya - y0;
  T cd = high ? (v3 - v1) : (v2 - v0);
  T k0 = cd / two;
  k0 = low ? -k0 : k0;
  T k1n = (v3 - v1) / two;
  // multicubic/regular.rs:528, :549, :583, :605 and multicubic/regular_recursive.rs:519, :570, :592
  T k1e = mul_add<FMA>(two, dy, -k0);
  if constexpr (ARMS && FMA) {
    if (d.k1_plain) k1e = two * dy - k0;  // multicubic/regular_recursive.rs:536
  }
  T k1 = (low || high) ? k1e : k1n;
  if (d.linear) {
    val = mul_add<FMA>(k1, d.tt - one, ya);  // multicubic/regular.rs:560, :616, multicubic/regular_recursive.rs:547, :603
    der = k1;
    return;
  }
  const HermiteCoef<T> c = hermite_coef<T>(y0, dy, k0, k1);
  val = hermite_eval<FMA, T>(d.tt, c.y0, c.c1, c.c2, c.c3);
  der = hermite_deriv<FMA, T>(d.tt, c.c1, c.c2, c.c3);
}

// The same on a rectilinear grid: cubic_rect_node's operations (ARMS: that function's; the derivative node uses the same k1).
template <bool FMA, typename T, bool ARMS = false>
__device__ __forceinline__ void cubic_rect_node_vd(T v0, T v1, T v2, T v3, const CubicDimRect<T>& d, T& val, T& der) {
  const T two = (T)2, one = (T)1;
  T y0, y1, dy, k0, k1;
  if (d.sat == kSatNone) {
    y0 = v1;
    y1 = v2;
    dy = v2 - v1;
    k0 = cd_unit_b<FMA>(v0, v1, v2, d.r0, d.a0, d.c0);
    k1 = cd_unit_a<FMA>(v1, v2, v3, d.r1, d.a1, d.c1);
  } else {
    cubic_rect_saturated<FMA, T>(v0, v1, v2, v3, d, y0, y1, dy, k0);
    k1 = two * dy - k0;  // multicubic/rectilinear.rs:471, :493, :515, :532 and multicubic/rectilinear_recursive.rs:469, :519: never fused
    if constexpr (ARMS && FMA) {
      if (d.fma_linear & kRectFuseK1) k1 = dev_fma<T>(two, dy, -k0);  // multicubic/rectilinear_recursive.rs:447, :502
    }
    if (d.linear) {
      if (FMA && d.fma_linear) {  // multicubic/rectilinear_recursive.rs:482, :532
        val = dev_fma<T>(k1, d.t - one, y1);
      } else {
        T p = k1 * (d.t - one);
        val = y1 + p;  // multicubic/rectilinear.rs:500, :539
      }
      der = k1;
      return;
    }
  }
  const HermiteCoef<T> c = hermite_coef<T>(y0, dy, k0, k1);
  val = hermite_eval<FMA, T>(d.t, c.y0, c.c1, c.c2, c.c3);
  der = hermite_deriv<FMA, T>(d.t, c.c1, c.c2, c.c3);
}

template <bool RECT, bool FMA, typename T>
__device__ __forceinline__ void cubic_node_vd(T v0, T v1, T v2, T v3, const typename CubicDimSel<T, RECT>::type& d, T& val, T& der) {
  if constexpr (RECT) cubic_rect_node_vd<FMA, T>(v0, v1, v2, v3, d, val, der);
  else cubic_regular_node_vd<FMA, T>(v0, v1, v2, v3, d, val, der);
}

// The spacing a rectilinear arm's t was divided by: h12 (None), h01 (Low), h23 (High) — cubic_rect_dim_setup's own
// subtractions on the same coordinates.
template <typename T, typename GridPtr>
__device__ __forceinline__ T cubic_rect_width(GridPtr g, int loc, int sat) {
  if (sat == kSatNone) return g[loc + 2] - g[loc + 1];
  return sat == kSatLow ? g[loc + 1] - g[loc] : g[loc + 3] - g[loc + 2];
}

template <typename T, int N>
struct CubicGradArgs {
  const T* bricks;
  unsigned table_bytes;  // < 4 GiB
  const T* obs[N];
  T* out;
  T* grad[N];
  unsigned long long* first_bad;
  size_t npts;
  T start[N];
  T step[N];
  int n[N];
  AxisArgs<T, N> ax;
  unsigned plane_stride[N];  // d >= 2: table elements per unit index of dim d
  unsigned nbj;
  int linearize;
};

// dims 0 and 1 of one tile (v[e], e = ei * 4 + ej): the value, d/dx0 and d/dx1 of the plane
template <typename T, bool RECT, bool FMA>
__device__ __forceinline__ void grad_reduce_tile(const T (&v)[16], const typename CubicDimSel<T, RECT>::type* dim, T& val, T& g0, T& g1) {
  T w[4], u[4];
#pragma unroll
  for (int ej = 0; ej < 4; ++ej) cubic_node_vd<RECT, FMA, T>(v[ej], v[4 + ej], v[8 + ej], v[12 + ej], dim[0], w[ej], u[ej]);
  cubic_node_vd<RECT, FMA, T>(w[0], w[1], w[2], w[3], dim[1], val, g1);
  g0 = cubic_node_sel<RECT, FMA, T>(u[0], u[1], u[2], u[3], dim[1]);
}

// One plane through the 16-lane transpose gather (gather_plane of cubic_brick.h without its reduction).
template <typename T>
__device__ __forceinline__ void grad_gather_tile(__amdgpu_buffer_rsrc_t bricks, const unsigned* toff, unsigned delta,
                                                 T __attribute__((may_alias))* lds_data, unsigned group, unsigned me, T (&v)[16]) {
  T val[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) val[r] = table_load<T>(bricks, toff[r], delta);  // byte offsets
#pragma unroll
  for (int r = 0; r < 16; ++r) lds_data[(group * 16 + r) * kCubRow + me] = val[r];
  wave_sync();
  const T __attribute__((may_alias))* row = lds_data + (group * 16 + me) * kCubRow;
#pragma unroll
  for (int e = 0; e < 16; ++e) v[e] = row[e];
  wave_sync();
}

template <typename T, int N, bool RECT, bool FMA, int SI, int SJ>
__global__ void __launch_bounds__(kBlock) k_cubic_grad(const CubicGradArgs<T, N> a) {
  static_assert(N == 2 || N == 3, "fused multicubic gradient kernel: N = 2, 3");
  INTERPN_CUBIC_BRICK_PROLOGUE()
  const size_t nthreads = (size_t)gridDim.x * kBlock;
  const size_t niter = (a.npts + nthreads - 1) / nthreads;
  for (size_t it = 0; it < niter; ++it) {
    // every lane runs every iteration: dead lanes take part in the gathers' exchanges with the offsets of a valid point
    const size_t i0 = it * nthreads + (size_t)blockIdx.x * kBlock + lane;
    const bool live = i0 < a.npts;
    INTERPN_CUBIC_GRAD_CELL(live ? stream_load(a.obs[d] + i0) : (RECT ? (T)0 : a.start[d]), live, i0)
    if (live) {
      stream_store(a.out + i0, res);
#pragma unroll
      for (int d = 0; d < N; ++d) {
        const T s = INTERPN_CUBIC_GRAD_SIGNED(d);
        stream_store(a.grad[d] + i0, s / width[d]);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Runtime-N form on the C-ordered grid.
template <typename T>
struct CubicGradGenericArgs {
  const T* vals;
  const T* obs[kMaxDims];
  T* out;
  T* grad[kMaxDims];
  unsigned long long* first_bad;
  size_t npts;
  int ndims;
  T start[kMaxDims];
  T step[kMaxDims];
  const T* grid[kMaxDims];
  int n[kMaxDims];
  unsigned long long stride[kMaxDims];
  int linearize;
  int fma_linear;  // the reference's recursive arm (N >= 5), as in GenericArgs
};

// Out-of-line node of the runtime-N kernel: I (deriv == 0) or D (deriv != 0) of the node (keeps its code size bounded).
template <bool FMA, typename T>
__device__ __attribute__((noinline)) T cubic_grad_regular_node_ool(T v0, T v1, T v2, T v3, int sat, int linear, int k1_plain, T tt, int deriv) {
  CubicDimRegular<T> dr;
  dr.sat = sat; dr.linear = linear; dr.k1_plain = k1_plain; dr.tt = tt;
  T val, der;
  cubic_regular_node_vd<FMA, T, true>(v0, v1, v2, v3, dr, val, der);
  return deriv ? der : val;
}
template <bool FMA, typename T>
__device__ __attribute__((noinline)) T cubic_grad_rect_node_ool(T v0, T v1, T v2, T v3, int sat, int linear, int fma_linear,
                                                                T t, T r0, T a0, T c0, T r1, T a1, T c1, int deriv) {
  CubicDimRect<T> dr;
  dr.sat = sat; dr.linear = linear; dr.fma_linear = fma_linear; dr.t = t;
  dr.r0 = r0; dr.a0 = a0; dr.c0 = c0; dr.r1 = r1; dr.a1 = a1; dr.c1 = c1;
  T val, der;
  cubic_rect_node_vd<FMA, T, true>(v0, v1, v2, v3, dr, val, der);
  return deriv ? der : val;
}

template <typename T, int KIND, bool FMA>
__global__ void __launch_bounds__(kBlock) k_cubic_grad_n(const CubicGradGenericArgs<T> a) {
  const int N = a.ndims;
  const size_t nthreads = (size_t)gridDim.x * kBlock;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < a.npts; i += nthreads) {
    int c_sat[kMaxDims], c_lin[kMaxDims], c_plain[kMaxDims];  // c_plain: k1_plain (regular), CubicDimRect::fma_linear (rectilinear)
    T c_t[kMaxDims], c_w[kMaxDims];
    T rc_r0[kMaxDims], rc_a0[kMaxDims], rc_c0[kMaxDims], rc_r1[kMaxDims], rc_a1[kMaxDims], rc_c1[kMaxDims];
    unsigned long long base = 0;
    bool ok = true;
    for (int d = 0; d < N; ++d) {
      const T x = a.obs[d][i];
      int loc;
      if constexpr (KIND == kRegular) {
        T floc;
        ok &= regular_floc<T>(x, a.start[d], a.step[d], &floc);
        ok &= floc != (T)-9223372036854775808.0;
        INTERPN_CUBIC_CLASS(floc, a.start[d], a.step[d], a.n[d])
        loc = l;
        const T t = (x - index_one_loc) / a.step[d];
        c_sat[d] = sat;
        c_lin[d] = (outside && a.linearize) ? 1 : 0;
        c_plain[d] = (a.fma_linear != 0 && sat == kSatLow && outside) ? 1 : 0;  // recursive arm's OutsideLow (regular_recursive.rs:536)
        c_t[d] = INTERPN_CUBIC_TT(t);
        c_w[d] = a.step[d];
      } else {
        Axis<T> ax;
        ax.g = a.grid[d]; ax.tab = nullptr; ax.n = a.n[d]; ax.M = 0; ax.g0 = (T)0; ax.scale = (T)0;
        CubicDimRect<T> dr;
        loc = cubic_rect_locate<T>(ax, x, a.linearize, a.fma_linear != 0, dr);
        c_sat[d] = dr.sat; c_lin[d] = dr.linear; c_plain[d] = dr.fma_linear; c_t[d] = dr.t;
        rc_r0[d] = dr.r0; rc_a0[d] = dr.a0; rc_c0[d] = dr.c0;
        rc_r1[d] = dr.r1; rc_a1[d] = dr.a1; rc_c1[d] = dr.c1;
        c_w[d] = cubic_rect_width<T>(a.grid[d], loc, dr.sat);
      }
      base += (unsigned long long)loc * a.stride[d];
    }
    if (!ok) atomicMin(a.first_bad, (unsigned long long)i);

    auto node = [&](const T* v, int d, int deriv) -> T {
      if constexpr (KIND == kRegular)
        return cubic_grad_regular_node_ool<FMA, T>(v[0], v[1], v[2], v[3], c_sat[d], c_lin[d], c_plain[d], c_t[d], deriv);
      else
        return cubic_grad_rect_node_ool<FMA, T>(v[0], v[1], v[2], v[3], c_sat[d], c_lin[d], c_plain[d], c_t[d], rc_r0[d],
                                                rc_a0[d], rc_c0[d], rc_r1[d], rc_a1[d], rc_c1[d], deriv);
    };

    // pass -1: the value (k_generic's vertex loop); pass p: component p, the same walk with D at level p
    const unsigned long long nverts = 1ull << (2 * N);
    for (int pass = -1; pass < N; ++pass) {
      T store[kMaxDims][4];
      for (unsigned long long v = 0; v < nverts; ++v) {
        unsigned long long idx = base;
        for (int k = 0; k < N; ++k) idx += ((v >> (2 * k)) & 3ull) * a.stride[k];
        store[0][v & 3ull] = a.vals[idx];
        for (int j = 1; j < N; ++j) {
          const unsigned long long q = 1ull << (2 * j);
          if (((v + 1) & (q - 1)) == 0) {
            const int p = (int)((((v + 1) >> (2 * j)) - 1) & 3ull);
            store[j][p] = node(store[j - 1], j - 1, pass == j - 1);
          }
        }
      }
      const T r = node(store[N - 1], N - 1, pass == N - 1);
      if (pass < 0) a.out[i] = r;
      else a.grad[pass][i] = (c_sat[pass] == kSatLow ? -r : r) / c_w[pass];
    }
  }
}

}  // namespace interpn
