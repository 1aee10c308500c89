// Values AND Jacobian of a field set on a lattice (lattice.h, "Field-set gradients on a lattice"): the product of
// k_lattice_fields_rows (k_lattice_fields.hip: the field loop around a row, groups of G fields, the fields-last tile) and
// k_lattice_grad_rows (lattice_grad.h: L lines per field, the width, sign and division of every component).
//
// Nothing new is defined.  For field f and the lattice point p in C order the value has the bits of k_lattice_fields_rows
// for field f, and component d of the Jacobian those of grad[d][p] of k_lattice_grad_rows on field f alone: the column
// loop and the output statements below are that kernel's, applied to `vals + (f0 + f) * field_stride` and to the field's
// own L lines, with the records of ONE launch of k_lattice_axes (they do not depend on the field).
//
// What a group shares: the row's records of dims 0 .. N-2 with their widths and signs (once per row), and per output the
// last axis's record, width and sign (once per lane and chunk, where K single-field launches load them K times).
#pragma once

#include "lattice_grad.h"

namespace interpn {

template <typename T, int N>
struct LatticeFieldsGradRowsArgs {
  LatticeRowsArgs<T, N> r;   // vals: field 0; out: the values; line_bytes: unused (a wave's lines lie n_last elements apart)
  T* jac;
  const T* grid[N];          // rectilinear: the set's axes (device)
  T step[N];                 // regular
  size_t field_stride;       // elements from field to field in `vals`
  size_t out_stride;         // field-major: elements from field to field; fields-last: from point to point
  size_t jac_stride;         // field-major: elements from (f, d) to (f, d + 1); fields-last: from point to point
  unsigned nfields;
  unsigned group;            // G: fields per pass over a row
  unsigned wave_bytes;       // LDS bytes from wave to wave: G * L lines, then the tile (fields-last)
  unsigned tile_off;         // bytes from a wave's first line to its tile
};

// One element of a fields-last tile to global memory.  `whole` (launch-uniform: G == K): a pass writes a point's whole run
// of K and of K * N elements, every byte of a line is written once, and the store is a stream like every other result
// store.  G < K: a line is completed by K / G passes that lie a row pass apart, and a non-temporal partial write of it
// costs a memory transaction each time; written as ordinary stores the passes meet in the cache.  Measured, one process
// alternating both builds (3-D 64^3 -> 256^3 f64, K = 3, G = 1: 1.92 -> 1.13 ms; multicubic 160^3: 0.55 -> 0.33 ms; f32
// K = 4, G = 2: 0.95 -> 0.59 ms; with G = K = 3 the stream is the faster one, 0.36 against 0.38 ms): DESIGN.md section 20.
template <typename T>
__device__ __forceinline__ void tile_store(bool whole, T* p, T v) {
  if (whole) stream_store(p, v);
  else *p = v;
}

// LAST is a template parameter for the reason given at k_lattice_fields_rows: the two stores differ in structure.
template <typename T, int METHOD, int N, bool RECT, bool FMA, bool LAST>
__global__ void __launch_bounds__(kLatticeBlock) k_lattice_fields_grad_rows(const LatticeFieldsGradRowsArgs<T, N> fa) {
  static_assert(N == 2 || N == 3, "row kernel: N = 2, 3");
  constexpr unsigned L = METHOD == kLinear ? N + 1 : N;  // lattice_grad_lines
  typedef typename LatticeRec<T, METHOD, RECT>::type Rec;
  typedef LatticeDim<T, METHOD, RECT> Dim;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const LatticeRowsArgs<T, N>& a = fa.r;
  const unsigned lane = threadIdx.x & 63u;
  const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const unsigned n_last = (unsigned)a.n_last;
  // lines of the wave: per field of the group r, a_0 (, a_1), and for multilinear handles b
  T* lines = reinterpret_cast<T*>(smem_raw + (size_t)wave * fa.wave_bytes);
  T* tile = reinterpret_cast<T*>(smem_raw + (size_t)wave * fa.wave_bytes + fa.tile_off);  // fields-last only
  const unsigned field_lines = L * n_last;  // elements from field to field of the group
  [[maybe_unused]] const bool whole = fa.group >= fa.nfields;  // fields-last: one pass writes a point's whole run (tile_store)
  const Rec* recs = static_cast<const Rec*>(a.recs);
  const Rec* recs_last = recs + a.rec_off[N - 1];
  const unsigned m_last = a.m[N - 1];
  const T* grid_last = fa.grid[N - 1];
  const T step_last = fa.step[N - 1];
  const unsigned long long row_step = (unsigned long long)gridDim.x * kLatticeWaves;
  for (unsigned long long row = (unsigned long long)blockIdx.x * kLatticeWaves + wave; row < a.nrows; row += row_step) {
    // the row's records of dims 0 .. N-2, their widths and signs: the same for every lane and every field
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
        width[d] = lattice_grad_width<T, RECT>(dim[d], fa.grid[d], fa.step[d]);
        neg[d] = lattice_grad_negative<T, RECT>(dim[d]);
      }
    }
    const unsigned long long p_row = row * m_last;  // flat index of the row's first point
    for (unsigned f0 = 0; f0 < fa.nfields; f0 += fa.group) {
      const unsigned gw = fa.nfields - f0 < fa.group ? fa.nfields - f0 : fa.group;  // the last pass may be short
      // field f of the group: its L lines at grid column k of the last axis (k_lattice_grad_rows' statements)
      for (unsigned f = 0; f < gw; ++f) {
        const T* field = a.vals + (size_t)(f0 + f) * fa.field_stride;
        T* line_r = lines + f * field_lines;
        T* line_a = line_r + n_last;                // a_d: line_a + d * n_last
        T* line_b = line_r + (unsigned)N * n_last;  // multilinear only
        for (unsigned k = lane; k < n_last; k += 64u) {
          const T* col = field + base + k;
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
      }
      wave_sync();
      // the row's outputs in chunks of 64: the last axis's record, width and sign once, then per field of the group the
      // value node and the N components from that field's lines (k_lattice_grad_rows' statements)
      for (unsigned j0 = 0; j0 < m_last; j0 += 64u) {
        const unsigned here = m_last - j0 < 64u ? m_last - j0 : 64u;
        const unsigned j = j0 + (lane < here ? lane : here - 1u);  // lanes behind a ragged chunk repeat its last record
        Dim last;
        last.load(recs_last[j]);
        const T h_last = lattice_grad_width<T, RECT>(last, grid_last, step_last);
        const unsigned ts = (fa.group * (unsigned)(N + 1)) | 1u;  // the tile's pitch
        for (unsigned f = 0; f < gw; ++f) {
          const T* line_r = lines + f * field_lines;
          const T* line_a = line_r + n_last;
          const T* line_b = line_r + (unsigned)N * n_last;
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
          if constexpr (!LAST) {
            // N + 1 coalesced stores per field; addresses from the two bases and strides in 64 bits
            if (lane < here) {
              const unsigned long long p = p_row + j;
              stream_store(a.out + (size_t)(f0 + f) * fa.out_stride + p, res);
              T* dj = fa.jac + (size_t)(f0 + f) * (size_t)N * fa.jac_stride + p;
#pragma unroll
              for (int d = 0; d < N - 1; ++d) stream_store(dj + (size_t)d * fa.jac_stride, g[d] / width[d]);
              stream_store(dj + (size_t)(N - 1) * fa.jac_stride, gl / h_last);
            }
          } else {
            // the lane's tile row: G values, then G x N Jacobian elements
            T* tr = tile + lane * ts;
            tr[f] = res;
            T* tj = tr + fa.group + f * (unsigned)N;
#pragma unroll
            for (int d = 0; d < N - 1; ++d) tj[d] = g[d] / width[d];
            tj[N - 1] = gl / h_last;
          }
        }
        if constexpr (LAST) {
          wave_sync();
          // lane-contiguous stores with k_lattice_fields_rows' element walk: the values, element e = (point e / gw, field
          // e % gw); then the Jacobian, element e = (point e / (gw * N), index e % (gw * N))
          {
            const unsigned q = 64u / gw, r = 64u - q * gw;  // uniform: what 64 more elements add to (point, field)
            unsigned p = lane / gw;
            unsigned f = lane - p * gw;
            T* dst = a.out + (size_t)(p_row + j0) * fa.out_stride + f0;
            for (unsigned k = 0; k < gw; ++k) {
              if (p < here) tile_store(whole, dst + (size_t)p * fa.out_stride + f, tile[p * ts + f]);
              p += q;
              f += r;
              if (f >= gw) {
                f -= gw;
                ++p;
              }
            }
          }
          {
            const unsigned gn = gw * (unsigned)N;
            const unsigned q = 64u / gn, r = 64u - q * gn;
            unsigned p = lane / gn;
            unsigned e = lane - p * gn;
            T* dst = fa.jac + (size_t)(p_row + j0) * fa.jac_stride + (size_t)f0 * (size_t)N;
            for (unsigned k = 0; k < gn; ++k) {
              if (p < here) tile_store(whole, dst + (size_t)p * fa.jac_stride + e, tile[p * ts + fa.group + e]);
              p += q;
              e += r;
              if (e >= gn) {
                e -= gn;
                ++p;
              }
            }
          }
          wave_sync();  // the next chunk overwrites the tile
        }
      }
      wave_sync();  // the next group, or the next row, overwrites the lines
    }
  }
}

}  // namespace interpn
