// Multilinear value AND gradient (d/dx of every point) in one pass.
//
// The gradient of a multilinear interpolant comes from the same 2^N corner values the value needs: component d is the
// difference of the two faces of the cell across dimension d, reduced over the other dimensions like the value, divided
// by the cell's width (DESIGN.md "Gradients" holds the definition the kernels are tested against bit for bit):
//   W[c']   = V[c' | 1 << d] - V[c']           one subtraction per corner pair
//   s       = W reduced over e != d, ascending e, with the reference's lerp(t[e], y0, y1)
//   grad[d] = s / h[d]                          IEEE division; h = steps[d], or x1 - x0 of the point's cell
//
//   k_linear_grad<T, N, RECT, FMA, SI, SJ, PPL, AXR, CELL>   N = 2, 3: gathers from the re-laid table the handle already
//       has — the 2-D bricks with k_linear2_brick's lane-pair gather, the 3-D bricks (steps SI, SJ; CELL == 2: the f32
//       2 x 4 x 4 bricks) with linear_brick.h's quad gather — so a gradient call reads the table lines of a value call
//       and adds N output streams.  Cell search, t and the value are the value kernels' operations: `out` has eval's bits.
//       Prologue, cell search, gather, value tree and gradient arithmetic are the shared cell body of linear_cell.h; the
//       kernel's own are the loads of the N coordinate arrays and the stores of the value and the N components.
//   k_linear_grad_n<T, KIND, FMA>   runtime N = 1..8 on the C-ordered grid: everything else.  One pass over the 2^N
//       corners for the value and one over the 2^(N-1) pairs of every component; written for correctness, not tuned.
#pragma once

#include "linear_cell.h"

namespace interpn {

template <typename T, int N>
struct GradArgs {
  const T* bricks;
  const T* obs[N];
  T* out;
  T* grad[N];
  unsigned long long* first_bad;
  size_t npts;
  T start[N];
  T step[N];
  int n[N];
  AxisArgs<T, N> ax;
  unsigned nbj, nbk;  // N == 3: bricks along j and k; N == 2: nbj = bricks along j
  unsigned iters;     // kBlock-wide iterations per workgroup
};

template <typename T, int N, bool RECT, bool FMA, int SI, int SJ, int PPL, int AXR = 0, int CELL = 0>
__global__ void __launch_bounds__(kBlock) k_linear_grad(const GradArgs<T, N> a) {
  static_assert(N == 2 || N == 3, "fused gradient kernel: N = 2, 3");
  static_assert(CELL == 0 || (CELL == 2 && N == 3 && sizeof(T) == 4 && SI == 1 && SJ == 1), "2 x 4 x 4 bricks: 3-D f32");
  INTERPN_CELL_PROLOGUE();
  const unsigned lane = threadIdx.x;
  const size_t nslots = (a.npts + PPL - 1) / PPL;
  const size_t first = (size_t)blockIdx.x * a.iters * kBlock;
  typedef T TV __attribute__((ext_vector_type(PPL >= 2 ? PPL : 2)));
  for (unsigned it = 0; it < a.iters; ++it) {
    // every lane runs every iteration (dead lanes still fetch pieces for their quad / pair)
    const size_t s0 = first + (size_t)it * kBlock + lane;
    if (s0 - lane >= nslots) break;  // block-uniform
    const size_t i0 = s0 * PPL;
    T xin[PPL][N];
    bool live[PPL];
#pragma unroll
    for (int h = 0; h < PPL; ++h) live[h] = i0 + h < a.npts;
    if constexpr (PPL >= 2) {
#pragma unroll
      for (int d = 0; d < N; ++d) {
        TV v;
#pragma unroll
        for (int h = 0; h < PPL; ++h) v[h] = RECT ? (T)0 : a.start[d];
        if (live[PPL - 1]) {
          v = stream_load(reinterpret_cast<const TV*>(a.obs[d] + i0));
        } else {  // the batch's ragged tail
#pragma unroll
          for (int h = 0; h < PPL; ++h)
            if (live[h]) v[h] = stream_load(a.obs[d] + i0 + h);
        }
#pragma unroll
        for (int h = 0; h < PPL; ++h) xin[h][d] = v[h];
      }
    } else {
#pragma unroll
      for (int d = 0; d < N; ++d) xin[0][d] = live[0] ? stream_load(a.obs[d] + i0) : (RECT ? (T)0 : a.start[d]);
    }
    int cell_r[PPL][N];
    T x0_r[PPL][N], x1_r[PPL][N];
    if constexpr (RECT && AXR != 0) lane_axes_locate<T, N, PPL, AXR>(a.ax, la, xin, cell_r, x0_r, x1_r);
    T resv[PPL], gradv[N][PPL];
#pragma unroll
    for (int h = 0; h < PPL; ++h) {
      INTERPN_CELL_SEARCH(xin[h], cell_r[h], x0_r[h], x1_r[h], live[h], i0 + h);
      if constexpr (N == 3) {
        INTERPN_CELL_VALUE3(resv[h]);
        INTERPN_CELL_GRAD3(gradv[0][h], gradv[1][h], gradv[2][h]);
      } else {
        INTERPN_CELL_VALUE2(resv[h]);
        INTERPN_CELL_GRAD2(gradv[0][h], gradv[1][h]);
      }
    }
    if constexpr (PPL >= 2) {
      if (live[PPL - 1]) {
        TV v;
#pragma unroll
        for (int h = 0; h < PPL; ++h) v[h] = resv[h];
        stream_store(reinterpret_cast<TV*>(a.out + i0), v);
#pragma unroll
        for (int d = 0; d < N; ++d) {
#pragma unroll
          for (int h = 0; h < PPL; ++h) v[h] = gradv[d][h];
          stream_store(reinterpret_cast<TV*>(a.grad[d] + i0), v);
        }
      } else {
#pragma unroll
        for (int h = 0; h < PPL; ++h)
          if (live[h]) {
            stream_store(a.out + i0 + h, resv[h]);
#pragma unroll
            for (int d = 0; d < N; ++d) stream_store(a.grad[d] + i0 + h, gradv[d][h]);
          }
      }
    } else if (live[0]) {
      stream_store(a.out + i0, resv[0]);
#pragma unroll
      for (int d = 0; d < N; ++d) stream_store(a.grad[d] + i0, gradv[d][0]);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Runtime-N form on the C-ordered grid.
template <typename T>
struct GradGenericArgs {
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
  int fma_index;  // regular grids: index_zero_loc fused (the reference's flattened arm, N <= 6; k_generic)
};

template <typename T, int KIND, bool FMA>
__global__ void __launch_bounds__(kBlock) k_linear_grad_n(const GradGenericArgs<T> a) {
  const int N = a.ndims;
  const size_t nthreads = (size_t)gridDim.x * kBlock;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < a.npts; i += nthreads) {
    T t[kMaxDims], width[kMaxDims];
    unsigned long long base = 0;
    bool ok = true;
    for (int d = 0; d < N; ++d) {
      const T x = a.obs[d][i];
      int loc;
      if constexpr (KIND == kRegular) {
        T floc;
        ok &= regular_floc<T>(x, a.start[d], a.step[d], &floc);
        loc = clamp_loc<T>(floc, a.n[d] - 2);
        const T izl = (FMA && a.fma_index) ? dev_fma<T>(a.step[d], (T)loc, a.start[d])
                                           : mul_add<false>(a.step[d], (T)loc, a.start[d]);
        t[d] = (x - izl) / a.step[d];
        width[d] = a.step[d];
      } else {
        const T* g = a.grid[d];
        loc = partition_point_lt<T>(g, a.n[d], x) - 1;
        loc = loc > 0 ? loc : 0;
        loc = loc < a.n[d] - 2 ? loc : a.n[d] - 2;
        const T x0 = g[loc];
        const T x1 = g[loc + 1];
        const T step = x1 - x0;
        t[d] = (x - x0) / step;
        width[d] = step;
      }
      base += (unsigned long long)loc * a.stride[d];
    }
    if (!ok) atomicMin(a.first_bad, (unsigned long long)i);
    // pass -1: the value over all N dimensions (k_generic's vertex loop); pass d: component d, the corner pairs across
    // dimension d reduced over the other N - 1 dimensions in ascending order
    for (int pass = -1; pass < N; ++pass) {
      int dims[kMaxDims];  // the dimensions this pass reduces over, ascending
      int m = 0;
      for (int e = 0; e < N; ++e)
        if (e != pass) dims[m++] = e;
      const unsigned long long across = pass < 0 ? 0ull : a.stride[pass];
      T store[kMaxDims + 1][2];
      T val = (T)0;
      const unsigned nverts = 1u << m;
      for (unsigned v = 0; v < nverts; ++v) {
        unsigned long long idx = base;
        for (int k = 0; k < m; ++k) idx += (unsigned long long)((v >> k) & 1u) * a.stride[dims[k]];
        val = pass < 0 ? a.vals[idx] : a.vals[idx + across] - a.vals[idx];
        // carry chain: level k holds the pair of dimension dims[k]
        for (int k = 0; k < m; ++k) {
          const unsigned bit = (v >> k) & 1u;
          store[k][bit] = val;
          if (!bit) break;
          val = cell_lerp<FMA>(t[dims[k]], store[k][0], store[k][1]);
        }
      }
      if (pass < 0) a.out[i] = val;
      else a.grad[pass][i] = val / width[pass];
    }
  }
}

}  // namespace interpn
