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
//   k_linear_grad_n<T, KIND, FMA>   runtime N = 1..8 on the C-ordered grid: everything else.  One pass over the 2^N
//       corners for the value and one over the 2^(N-1) pairs of every component; written for correctness, not tuned.
#pragma once

#include "linear_brick.h"

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

// the reference's interpolation step (multilinear/regular.rs:378-385)
template <bool FMA, typename T>
__device__ __forceinline__ T grad_lerp(T t, T y0, T y1) {
  const T dy = y1 - y0;
  return mul_add<FMA>(t, dy, y0);
}

// swap with the neighbouring lane (lane ^ 1): quad_perm [1,0,3,2] (dpp_swap1 of k_linear2_brick.hip, a translation unit that
// cannot be included here)
__device__ __forceinline__ unsigned grad_swap1(unsigned v) {
  return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true);
}
__device__ __forceinline__ float grad_swap1(float v) { return __uint_as_float(grad_swap1(__float_as_uint(v))); }
__device__ __forceinline__ double grad_swap1(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = grad_swap1((unsigned)b), hi = grad_swap1((unsigned)(b >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

template <typename T, int N, bool RECT, bool FMA, int SI, int SJ, int PPL, int AXR = 0, int CELL = 0>
__global__ void __launch_bounds__(kBlock) k_linear_grad(const GradArgs<T, N> a) {
  static_assert(N == 2 || N == 3, "fused gradient kernel: N = 2, 3");
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
      T t[N], width[N];
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
          width[d] = step;
          loc[d] = l;
        } else {
          T floc;
          ok &= regular_floc<T>(x, a.start[d], a.step[d], &floc);  // multilinear/regular.rs:415-418
          const int l = clamp_loc<T>(floc, a.n[d] - 2);             // regular.rs:420-422
          const T izl = mul_add<FMA>(a.step[d], (T)l, a.start[d]);  // regular.rs:334-337
          t[d] = (x - izl) / a.step[d];                             // regular.rs:339
          width[d] = a.step[d];
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
        // value: the tree of k_linear_brick (i first, k last; multilinear/regular.rs:347-403)
        T r[2];
#pragma unroll
        for (int dk = 0; dk < 2; ++dk) {
          const T c0 = grad_lerp<FMA>(t[0], c.v[0][0][dk], c.v[1][0][dk]);
          const T c1 = grad_lerp<FMA>(t[0], c.v[0][1][dk], c.v[1][1][dk]);
          r[dk] = grad_lerp<FMA>(t[1], c0, c1);
        }
        resv[h] = grad_lerp<FMA>(t[2], r[0], r[1]);
        // d/dx0: differences along i, reduced over j then k
        T s[2];
#pragma unroll
        for (int dk = 0; dk < 2; ++dk)
          s[dk] = grad_lerp<FMA>(t[1], c.v[1][0][dk] - c.v[0][0][dk], c.v[1][1][dk] - c.v[0][1][dk]);
        gradv[0][h] = grad_lerp<FMA>(t[2], s[0], s[1]) / width[0];
        // d/dx1: differences along j, reduced over i then k
#pragma unroll
        for (int dk = 0; dk < 2; ++dk)
          s[dk] = grad_lerp<FMA>(t[0], c.v[0][1][dk] - c.v[0][0][dk], c.v[1][1][dk] - c.v[1][0][dk]);
        gradv[1][h] = grad_lerp<FMA>(t[2], s[0], s[1]) / width[1];
        // d/dx2: differences along k, reduced over i then j
#pragma unroll
        for (int dj = 0; dj < 2; ++dj)
          s[dj] = grad_lerp<FMA>(t[0], c.v[0][dj][1] - c.v[0][dj][0], c.v[1][dj][1] - c.v[1][dj][0]);
        gradv[2][h] = grad_lerp<FMA>(t[1], s[0], s[1]) / width[2];
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
        gradv[0][h] = grad_lerp<FMA>(t[1], row1.x - row0.x, row1.y - row0.y) / width[0];
        gradv[1][h] = grad_lerp<FMA>(t[0], row0.y - row0.x, row1.y - row1.x) / width[1];
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
          val = grad_lerp<FMA>(t[dims[k]], store[k][0], store[k][1]);
        }
      }
      if (pass < 0) a.out[i] = val;
      else a.grad[pass][i] = val / width[pass];
    }
  }
}

}  // namespace interpn
