// Device pieces of the lattice row kernels (lattice.h): the row arguments, a dimension's record as the node functions take
// it, and one node of the reference's reduction.  Shared by k_lattice_rows (k_lattice.hip) and k_lattice_fields_rows
// (k_lattice_fields.hip), so that a field of a set goes through the node functions of the single-field kernel.
#pragma once

#include "interpn_kernels.h"
#include "lattice.h"

namespace interpn {

template <typename T, int N>
struct LatticeRowsArgs {
  const T* vals;
  const void* recs;
  T* out;
  unsigned long long nrows;
  unsigned m[N];
  unsigned rec_off[N];
  unsigned stride[N];   // element strides of the C-ordered grid
  int n_last;
  unsigned line_bytes;  // LDS bytes from line to line
};

template <typename T, int METHOD, bool RECT> struct LatticeDim;
template <typename T, bool RECT>
struct LatticeDim<T, kLinear, RECT> {
  T t;
  int loc;
  __device__ __forceinline__ void load(const LatticeRecLinear<T>& r) { t = r.t; loc = r.loc; }
};
template <typename T>
struct LatticeDim<T, kCubic, false> {
  CubicDimRegular<T> d;
  int loc;
  __device__ __forceinline__ void load(const LatticeRecCubic<T>& r) {
    d.tt = r.tt; d.sat = r.cls & 3; d.linear = r.cls >> 2; d.k1_plain = 0;
    loc = r.loc;
  }
};
template <typename T>
struct LatticeDim<T, kCubic, true> {
  CubicDimRect<T> d;
  int loc;
  __device__ __forceinline__ void load(const LatticeRecCubicRect<T>& r) {
    d.sat = r.cls & 3; d.linear = r.cls >> 2; d.fma_linear = 0;  // the flattened arm never fuses the linearized branch
    d.t = r.t; d.r0 = r.r0; d.a0 = r.a0; d.c0 = r.c0; d.r1 = r.r1; d.a1 = r.a1; d.c1 = r.c1;
    d.rr0 = (T)1; d.rr1 = (T)1; d.fast = false;
    loc = r.loc;
  }
};

// One node of the reference's reduction: FP values of one dimension -> one.
template <bool FMA, typename T, bool RECT>
__device__ __forceinline__ T lattice_node(const T (&v)[2], const LatticeDim<T, kLinear, RECT>& s) {
  const T y0 = v[0];
  const T dy = v[1] - y0;
  return mul_add<FMA>(s.t, dy, y0);  // regular.rs:378-385 / rectilinear.rs:339-344
}
template <bool FMA, typename T>
__device__ __forceinline__ T lattice_node(const T (&v)[4], const LatticeDim<T, kCubic, false>& s) {
  return cubic_regular_node<FMA, T>(v[0], v[1], v[2], v[3], s.d);
}
template <bool FMA, typename T>
__device__ __forceinline__ T lattice_node(const T (&v)[4], const LatticeDim<T, kCubic, true>& s) {
  return cubic_rect_node<FMA, T>(v[0], v[1], v[2], v[3], s.d);
}

}  // namespace interpn
