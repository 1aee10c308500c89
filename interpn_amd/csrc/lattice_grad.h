// Value AND gradient on a lattice (lattice.h, "Gradients on a lattice"): k_lattice_rows with L lines per wave.
//
// Nothing new is defined.  For the lattice point p in C order `out[p]` has the bits of k_lattice_rows (and so of eval),
// and grad[d][p] those of component d of the per-point gradient kernels on the expanded point: linear_grad.h
// (DESIGN.md "Gradients") for multilinear handles, cubic_grad.h (DESIGN.md "Multicubic gradients") for multicubic ones.
//
// What a row shares.  The partial results of EVERY component after dimensions 0 .. N-2 depend only on the output row and
// on the grid column k of the last axis, as the value's do.  With the row's records of dimensions 0 .. N-2 and v(c, k) the
// table value at corner / footprint index c over those dimensions:
//   multilinear, L = N + 1 lines
//     r[k]     the value line of k_lattice_rows
//     a_d[k]   d < N-1: W[c'] = v(c' | 1 << d, k) - v(c', k), reduced over the dimensions e < N-1, e != d, ascending
//     b[k]     k < n_last - 1: W[c] = v(c, k + 1) - v(c, k), reduced over dimensions 0 .. N-2 like the value.  Not
//              r[k + 1] - r[k] in floating point: the definition subtracts first.
//     out = lerp(t, r[loc], r[loc+1]);  grad[d] = lerp(t, a_d[loc], a_d[loc+1]) / h_d;  grad[N-1] = b[loc] / h_{N-1}
//   multicubic, L = N lines: per column the tree of grad_reduce_tile (cubic_grad.h) on the C-ordered values
//     r[k]     the value;  a_d[k]: the derivative node D at level d, value nodes I elsewhere
//     (out, der) = cubic_node_vd(r[loc .. loc+3]);  grad[N-1] = +-der / h;  grad[d] = +-I_last(a_d[loc .. loc+3]) / h_d
// h_d: step[d] on a regular grid; on a rectilinear one the width of the coordinate's cell read from the handle's axis
// (multilinear: g[loc+1] - g[loc]; multicubic: cubic_rect_width).  The sign is negative for the Low class along d.  One
// IEEE division per component.  The records are k_lattice_axes', unchanged.
//
// Per output: one record load and N + 1 stores, each coalesced along the row — (N + 1) sizeof(T) bytes to HBM against
// (2 N + 1) sizeof(T) for the per-point kernels on an expanded lattice.
#pragma once

#include "cubic_grad.h"
#include "lattice_rows.h"

namespace interpn {

template <typename T, int N>
struct LatticeGradRowsArgs {
  LatticeRowsArgs<T, N> r;   // line_bytes: unused (the lines of a wave lie n_last elements apart)
  T* grad[N];
  const T* grid[N];          // rectilinear: the handle's axes (device)
  T step[N];                 // regular
  unsigned wave_bytes;       // LDS bytes from wave to wave
};

// The width and sign of a coordinate's component from its record as LatticeDim holds it.
template <typename T, bool RECT>
__device__ __forceinline__ T lattice_grad_width(const LatticeDim<T, kLinear, RECT>& s, const T* g, T step) {
  if constexpr (RECT) return g[s.loc + 1] - g[s.loc];  // rectilinear.rs:312
  else return step;
}
template <typename T, bool RECT>
__device__ __forceinline__ T lattice_grad_width(const LatticeDim<T, kCubic, RECT>& s, const T* g, T step) {
  if constexpr (RECT) return cubic_rect_width<T>(g, s.loc, s.d.sat);
  else return step;
}
template <typename T, bool RECT>
__device__ __forceinline__ bool lattice_grad_negative(const LatticeDim<T, kLinear, RECT>&) { return false; }
template <typename T, bool RECT>
__device__ __forceinline__ bool lattice_grad_negative(const LatticeDim<T, kCubic, RECT>& s) { return s.d.sat == kSatLow; }

template <typename T, int METHOD, int N, bool RECT, bool FMA>
__global__ void __launch_bounds__(kLatticeBlock) k_lattice_grad_rows(const LatticeGradRowsArgs<T, N> ga) {
  static_assert(N == 2 || N == 3, "row kernel: N = 2, 3");
  typedef typename LatticeRec<T, METHOD, RECT>::type Rec;
  typedef LatticeDim<T, METHOD, RECT> Dim;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const LatticeRowsArgs<T, N>& a = ga.r;
  const unsigned lane = threadIdx.x & 63u;
  const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const unsigned n_last = (unsigned)a.n_last;
  // lines of the wave: r, a_0 (, a_1), and for multilinear handles b
  T* line_r = reinterpret_cast<T*>(smem_raw + (size_t)wave * ga.wave_bytes);
  T* line_a = line_r + n_last;             // a_d: line_a + d * n_last
  T* line_b = line_r + (unsigned)N * n_last;  // multilinear only
  const Rec* recs = static_cast<const Rec*>(a.recs);
  const Rec* recs_last = recs + a.rec_off[N - 1];
  const unsigned m_last = a.m[N - 1];
  const T* grid_last = ga.grid[N - 1];
  const T step_last = ga.step[N - 1];
  const unsigned long long row_step = (unsigned long long)gridDim.x * kLatticeWaves;
  for (unsigned long long row = (unsigned long long)blockIdx.x * kLatticeWaves + wave; row < a.nrows; row += row_step) {
    // the row's records of dims 0 .. N-2, their widths and signs: the same for every lane
    Dim dim[N - 1];
    T width[N - 1];
    bool neg[N - 1];
    unsigned base = 0;
    {
      unsigned long long rest = row;
#pragma unroll
      for (int d = N - 2; d >= 0; --d) {
        const unsigned i = (unsigned)(rest % a.m[d]);
        rest /= a.m[d];
        dim[d].load(recs[a.rec_off[d] + i]);
        base += (unsigned)dim[d].loc * a.stride[d];
        width[d] = lattice_grad_width<T, RECT>(dim[d], ga.grid[d], ga.step[d]);
        neg[d] = lattice_grad_negative<T, RECT>(dim[d]);
      }
    }
    // the lines at grid column k of the last axis (dimension 0 innermost, as the reference's tree)
    for (unsigned k = lane; k < n_last; k += 64u) {
      const T* col = a.vals + base + k;
      if constexpr (METHOD == kLinear) {
        const bool more = k + 1 < n_last;  // b has n_last - 1 entries
        if constexpr (N == 2) {
          const T v0 = col[0], v1 = col[a.stride[0]];
          const T x[2] = {v0, v1};
          line_r[k] = lattice_node<FMA, T>(x, dim[0]);
          line_a[k] = v1 - v0;
          if (more) {
            const T w[2] = {col[1] - v0, col[a.stride[0] + 1] - v1};
            line_b[k] = lattice_node<FMA, T>(w, dim[0]);
          }
        } else {
          T v[2][2];  // v[i][j]
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i) v[i][j] = col[(unsigned)j * a.stride[1] + (unsigned)i * a.stride[0]];
          T w[2];
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const T x[2] = {v[0][j], v[1][j]};
            w[j] = lattice_node<FMA, T>(x, dim[0]);
          }
          line_r[k] = lattice_node<FMA, T>(w, dim[1]);
          // d/dx0: differences along i, reduced over j;  d/dx1: differences along j, reduced over i
          const T s0[2] = {v[1][0] - v[0][0], v[1][1] - v[0][1]};
          line_a[k] = lattice_node<FMA, T>(s0, dim[1]);
          const T s1[2] = {v[0][1] - v[0][0], v[1][1] - v[1][0]};
          line_a[n_last + k] = lattice_node<FMA, T>(s1, dim[0]);
          if (more) {
            // d/dx2: differences along k, reduced over i then j
            T u[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
              const T* nxt = col + 1 + (unsigned)j * a.stride[1];
              const T x[2] = {nxt[0] - v[0][j], nxt[a.stride[0]] - v[1][j]};
              u[j] = lattice_node<FMA, T>(x, dim[0]);
            }
            line_b[k] = lattice_node<FMA, T>(u, dim[1]);
          }
        }
      } else {
        if constexpr (N == 2) {
          T val, der;
          cubic_node_vd<RECT, FMA, T>(col[0], col[a.stride[0]], col[2u * a.stride[0]], col[3u * a.stride[0]], dim[0].d, val, der);
          line_r[k] = val;
          line_a[k] = der;
        } else {
          T w[4], u[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const T* p = col + (unsigned)j * a.stride[1];
            cubic_node_vd<RECT, FMA, T>(p[0], p[a.stride[0]], p[2u * a.stride[0]], p[3u * a.stride[0]], dim[0].d, w[j], u[j]);
          }
          T val, g1;
          cubic_node_vd<RECT, FMA, T>(w[0], w[1], w[2], w[3], dim[1].d, val, g1);
          line_r[k] = val;
          line_a[k] = cubic_node_sel<RECT, FMA, T>(u[0], u[1], u[2], u[3], dim[1].d);
          line_a[n_last + k] = g1;
        }
      }
    }
    wave_sync();
    // the row's outputs: nodes of the last dimension, operands from the lines
    const unsigned long long at = row * m_last;
    for (unsigned j = lane; j < m_last; j += 64u) {
      Dim last;
      last.load(recs_last[j]);
      const T h_last = lattice_grad_width<T, RECT>(last, grid_last, step_last);
      T res, gl, g[N - 1];
      if constexpr (METHOD == kLinear) {
        const T x[2] = {line_r[last.loc], line_r[last.loc + 1]};
        res = lattice_node<FMA, T>(x, last);  // regular.rs:396-402
#pragma unroll
        for (int d = 0; d < N - 1; ++d) {
          const T* la = line_a + (unsigned)d * n_last + last.loc;
          const T y[2] = {la[0], la[1]};
          g[d] = lattice_node<FMA, T>(y, last);
        }
        gl = line_b[last.loc];
      } else {
        const T* lr = line_r + last.loc;
        cubic_node_vd<RECT, FMA, T>(lr[0], lr[1], lr[2], lr[3], last.d, res, gl);  // multicubic/regular.rs:415-421 and D
        if (lattice_grad_negative<T, RECT>(last)) gl = -gl;
#pragma unroll
        for (int d = 0; d < N - 1; ++d) {
          const T* la = line_a + (unsigned)d * n_last + last.loc;
          const T s = cubic_node_sel<RECT, FMA, T>(la[0], la[1], la[2], la[3], last.d);
          g[d] = neg[d] ? -s : s;
        }
      }
      stream_store(a.out + at + j, res);
#pragma unroll
      for (int d = 0; d < N - 1; ++d) stream_store(ga.grad[d] + at + j, g[d] / width[d]);
      stream_store(ga.grad[N - 1] + at + j, gl / h_last);
    }
    wave_sync();  // the next row overwrites the lines
  }
}

}  // namespace interpn
