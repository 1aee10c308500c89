// Lattice evaluation kernels (lattice.h): per-coordinate records, the row kernel, and the expansion of a lattice slice
// into SoA coordinates for the handle's ordinary kernels.
#include "lattice_rows.h"

namespace interpn {

// ---------------------------------------------------------------------------
// k_lattice_axes: one thread per axis coordinate, all axes in one launch.
template <typename T>
struct LatticeAxesArgs {
  const T* axes[kMaxDims];
  const T* grid[kMaxDims];  // rectilinear: the handle's axes (device)
  unsigned long long weight[kMaxDims];
  unsigned rec_off[kMaxDims];
  T start[kMaxDims], step[kMaxDims];
  int n[kMaxDims];
  int ndims;
  unsigned total;  // sum of the axis lengths
  int linearize;
  int cubic;       // k_lattice_check: the multicubic kernels' additional condition (floc - 1 must not overflow isize)
  void* recs;
  unsigned char* bad;
  unsigned long long* first_bad;
};

// The axis a flat coordinate index belongs to, by selects (every per-axis argument stays in scalar registers).
template <typename T>
struct LatticeAxisPick {
  const T* axis;
  const T* grid;
  unsigned long long weight;
  unsigned off;
  T start, step;
  int n;
};
template <typename T>
__device__ __forceinline__ LatticeAxisPick<T> lattice_pick_axis(const LatticeAxesArgs<T>& a, unsigned c) {
  LatticeAxisPick<T> p = {a.axes[0], a.grid[0], a.weight[0], 0u, a.start[0], a.step[0], a.n[0]};
#pragma unroll
  for (int e = 1; e < kMaxDims; ++e) {
    if (e < a.ndims && c >= a.rec_off[e]) {
      p.axis = a.axes[e]; p.grid = a.grid[e]; p.weight = a.weight[e]; p.off = a.rec_off[e];
      p.start = a.start[e]; p.step = a.step[e]; p.n = a.n[e];
    }
  }
  return p;
}

// A bad coordinate at position j of axis d fails every lattice point that uses it; the first of them in C order is
// j * prod(m_e, e > d) (all other indices zero).
template <typename T>
__device__ __forceinline__ void lattice_report(const LatticeAxesArgs<T>& a, unsigned c, const LatticeAxisPick<T>& p, bool ok) {
  if (a.bad) a.bad[c] = ok ? 0 : 1;
  if (!ok) atomicMin(a.first_bad, (unsigned long long)(c - p.off) * p.weight);
}

template <typename T, int METHOD, bool RECT, bool FMA>
__global__ void __launch_bounds__(kBlock) k_lattice_axes(const LatticeAxesArgs<T> a) {
  typedef typename LatticeRec<T, METHOD, RECT>::type Rec;
  Rec* recs = static_cast<Rec*>(a.recs);
  for (unsigned c = blockIdx.x * kBlock + threadIdx.x; c < a.total; c += gridDim.x * kBlock) {
    const LatticeAxisPick<T> p = lattice_pick_axis<T>(a, c);
    const T x = p.axis[c - p.off];
    Rec r;
    if constexpr (RECT) {
      Axis<T> ax;
      ax.g = p.grid; ax.tab = nullptr; ax.n = p.n; ax.M = 0; ax.g0 = (T)0; ax.scale = (T)0;
      if constexpr (METHOD == kLinear) {
        T x0, x1;
        r.loc = axis_cell<T>(ax, x, &x0, &x1);  // rectilinear.rs:353-370, :310-311
        const T step = x1 - x0;
        r.t = (x - x0) / step;                  // rectilinear.rs:310-313
      } else {
        CubicDimRect<T> d;
        r.loc = cubic_rect_locate<T>(ax, x, a.linearize, /*fma_linear=*/false, d);  // rectilinear.rs:377-405 + the cell's ratios
        r.t = d.t; r.r0 = d.r0; r.a0 = d.a0; r.c0 = d.c0; r.r1 = d.r1; r.a1 = d.a1; r.c1 = d.c1;
        r.cls = d.sat | (d.linear << 2);
      }
    } else {
      T floc;
      bool ok = regular_floc<T>(x, p.start, p.step, &floc);  // regular.rs:415-418
      if constexpr (METHOD == kLinear) {
        r.loc = clamp_loc<T>(floc, p.n - 2);                                  // regular.rs:420-422
        const T index_zero_loc = mul_add<FMA>(p.step, (T)r.loc, p.start);     // regular.rs:334-339 (flattened arm: fused)
        r.t = (x - index_zero_loc) / p.step;
      } else {
        ok &= floc != (T)-9223372036854775808.0;  // `- 1` would overflow isize: the reference panics
        INTERPN_CUBIC_CLASS(floc, p.start, p.step, p.n)  // multicubic/regular.rs:440-466, :356-360
        r.loc = l;
        const T t = (x - index_one_loc) / p.step;
        r.tt = INTERPN_CUBIC_TT(t);
        r.cls = sat | ((outside && a.linearize) ? 4 : 0);
      }
      lattice_report<T>(a, c, p, ok);
    }
    recs[c] = r;
  }
}

// The failing-point part alone (regular grids, every method and N): what the expanded path needs.
template <typename T>
__global__ void __launch_bounds__(kBlock) k_lattice_check(const LatticeAxesArgs<T> a) {
  for (unsigned c = blockIdx.x * kBlock + threadIdx.x; c < a.total; c += gridDim.x * kBlock) {
    const LatticeAxisPick<T> p = lattice_pick_axis<T>(a, c);
    const T x = p.axis[c - p.off];
    T floc;
    bool ok = regular_floc<T>(x, p.start, p.step, &floc);
    if (a.cubic) ok &= floc != (T)-9223372036854775808.0;
    lattice_report<T>(a, c, p, ok);
  }
}

// ---------------------------------------------------------------------------
// k_lattice_rows
// (row arguments, LatticeDim and lattice_node: lattice_rows.h)
template <typename T, int METHOD, int N, bool RECT, bool FMA>
__global__ void __launch_bounds__(kLatticeBlock) k_lattice_rows(const LatticeRowsArgs<T, N> a) {
  static_assert(N == 2 || N == 3, "row kernel: N = 2, 3");
  constexpr int FP = METHOD == kLinear ? 2 : 4;
  typedef typename LatticeRec<T, METHOD, RECT>::type Rec;
  typedef LatticeDim<T, METHOD, RECT> Dim;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const unsigned lane = threadIdx.x & 63u;
  const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  T* line = reinterpret_cast<T*>(smem_raw + (size_t)wave * a.line_bytes);
  const Rec* recs = static_cast<const Rec*>(a.recs);
  const Rec* recs_last = recs + a.rec_off[N - 1];
  const unsigned m_last = a.m[N - 1];
  const unsigned long long row_step = (unsigned long long)gridDim.x * kLatticeWaves;
  for (unsigned long long row = (unsigned long long)blockIdx.x * kLatticeWaves + wave; row < a.nrows; row += row_step) {
    // the row's records of dims 0 .. N-2: the same for every lane
    Dim dim[N - 1];
    unsigned base = 0;
    {
      unsigned long long rest = row;
#pragma unroll
      for (int d = N - 2; d >= 0; --d) {
        const unsigned i = (unsigned)(rest % a.m[d]);
        rest /= a.m[d];
        dim[d].load(recs[a.rec_off[d] + i]);
        base += (unsigned)dim[d].loc * a.stride[d];
      }
    }
    // r[k]: dims 0 .. N-2 reduced at grid column k of the last axis (dimension 0 innermost, as the reference's tree)
    for (unsigned k = lane; k < (unsigned)a.n_last; k += 64u) {
      const T* col = a.vals + base + k;
      T r;
      if constexpr (N == 2) {
        T v[FP];
#pragma unroll
        for (int i = 0; i < FP; ++i) v[i] = col[(unsigned)i * a.stride[0]];
        r = lattice_node<FMA, T>(v, dim[0]);
      } else {
        T w[FP];
#pragma unroll
        for (int j = 0; j < FP; ++j) {
          T v[FP];
#pragma unroll
          for (int i = 0; i < FP; ++i) v[i] = col[(unsigned)j * a.stride[1] + (unsigned)i * a.stride[0]];
          w[j] = lattice_node<FMA, T>(v, dim[0]);
        }
        r = lattice_node<FMA, T>(w, dim[1]);
      }
      line[k] = r;
    }
    wave_sync();
    // the row's outputs: one node of the last dimension each, operands from the line
    T* dst = a.out + row * m_last;
    for (unsigned j = lane; j < m_last; j += 64u) {
      Dim last;
      last.load(recs_last[j]);
      T v[FP];
#pragma unroll
      for (int i = 0; i < FP; ++i) v[i] = line[last.loc + i];
      stream_store(dst + j, lattice_node<FMA, T>(v, last));  // regular.rs:396-402 / multicubic/regular.rs:415-421
    }
    wave_sync();  // the next row overwrites the line
  }
}

// ---------------------------------------------------------------------------
// k_lattice_expand
template <typename T>
struct LatticeExpandArgs {
  const T* axes[kMaxDims];
  T* dst[kMaxDims];
  unsigned long long m[kMaxDims];
  unsigned rec_off[kMaxDims];
  T subst[kMaxDims];
  const unsigned char* bad;
  unsigned long long begin, count;
  int ndims;
};

template <typename T>
__global__ void __launch_bounds__(kBlock) k_lattice_expand(const LatticeExpandArgs<T> a) {
  const unsigned long long nthreads = (unsigned long long)gridDim.x * kBlock;
  for (unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; i < a.count; i += nthreads) {
    unsigned long long p = a.begin + i;
#pragma unroll
    for (int d = kMaxDims - 1; d >= 0; --d) {
      if (d < a.ndims) {
        const unsigned long long j = p % a.m[d];
        p /= a.m[d];
        T x = a.axes[d][j];
        if (a.bad && a.bad[a.rec_off[d] + j]) x = a.subst[d];
        a.dst[d][i] = x;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Launchers
template <typename T>
static void fill_axes_args(const GridDesc& g, const LatticeShape& s, LatticeAxesArgs<T>& a) {
  a.ndims = s.ndims;
  a.total = (unsigned)s.coords;
  a.linearize = g.linearize;
  a.cubic = g.method == kCubic ? 1 : 0;
  for (int d = 0; d < kMaxDims; ++d) {
    const bool live = d < s.ndims;
    a.axes[d] = live ? static_cast<const T*>(s.axes[d]) : nullptr;
    a.grid[d] = live ? static_cast<const T*>(g.grid[d]) : nullptr;
    a.weight[d] = live ? s.weight[d] : 0;
    a.rec_off[d] = live ? s.rec_off[d] : 0;
    a.start[d] = live ? (T)g.start[d] : (T)0;
    a.step[d] = live ? (T)g.step[d] : (T)1;
    a.n[d] = live ? g.n[d] : 0;
  }
}

static unsigned coord_blocks(size_t coords) {
  size_t want = (coords + kBlock - 1) / kBlock;
  if (want < 1) want = 1;
  return (unsigned)(want < 4096 ? want : 4096);
}

template <typename T, int METHOD, bool RECT>
static hipError_t launch_axes_m(const LatticeAxesArgs<T>& a, bool fma, hipStream_t stream) {
  const unsigned blocks = coord_blocks(a.total);
  if (fma) hipLaunchKernelGGL((k_lattice_axes<T, METHOD, RECT, true>), dim3(blocks), dim3(kBlock), 0, stream, a);
  else hipLaunchKernelGGL((k_lattice_axes<T, METHOD, RECT, false>), dim3(blocks), dim3(kBlock), 0, stream, a);
  return hipGetLastError();
}

template <typename T>
static hipError_t launch_axes_t(const GridDesc& g, const LatticeShape& s, void* recs, unsigned char* bad,
                                unsigned long long* first_bad, hipStream_t stream) {
  LatticeAxesArgs<T> a;
  fill_axes_args<T>(g, s, a);
  a.recs = recs;
  a.bad = bad;
  a.first_bad = first_bad;
  if (!recs) {
    if (g.kind != kRegular) return hipSuccess;  // rectilinear grids never fail a point
    hipLaunchKernelGGL((k_lattice_check<T>), dim3(coord_blocks(a.total)), dim3(kBlock), 0, stream, a);
    return hipGetLastError();
  }
  const bool fma = g.fma != 0;
  if (g.method == kLinear)
    return g.kind == kRegular ? launch_axes_m<T, kLinear, false>(a, fma, stream) : launch_axes_m<T, kLinear, true>(a, fma, stream);
  if (g.method == kCubic)
    return g.kind == kRegular ? launch_axes_m<T, kCubic, false>(a, fma, stream) : launch_axes_m<T, kCubic, true>(a, fma, stream);
  return hipErrorInvalidValue;
}

hipError_t launch_lattice_axes(const GridDesc& g, const LatticeShape& s, void* recs, unsigned char* bad,
                               unsigned long long* first_bad, hipStream_t stream) {
  if (s.coords == 0) return hipSuccess;
  return g.dtype == kF64 ? launch_axes_t<double>(g, s, recs, bad, first_bad, stream)
                         : launch_axes_t<float>(g, s, recs, bad, first_bad, stream);
}

template <typename T, int METHOD, int N, bool RECT, bool FMA>
static hipError_t launch_rows_k(const GridDesc& g, const LatticeShape& s, const void* recs, void* out, size_t lds_bytes,
                                hipStream_t stream) {
  LatticeRowsArgs<T, N> a;
  a.vals = static_cast<const T*>(g.vals);
  a.recs = recs;
  a.out = static_cast<T*>(out);
  a.nrows = 1;
  unsigned acc = 1;
  for (int d = N - 1; d >= 0; --d) {
    a.m[d] = (unsigned)s.m[d];
    a.rec_off[d] = s.rec_off[d];
    a.stride[d] = acc;
    acc *= (unsigned)g.n[d];
    if (d < N - 1) a.nrows *= s.m[d];
  }
  a.n_last = g.n[N - 1];
  a.line_bytes = (unsigned)(lds_bytes / kLatticeWaves);
  const unsigned long long want = (a.nrows + kLatticeWaves - 1) / kLatticeWaves;
  const unsigned long long cap = (unsigned long long)g.cfg.num_cus * (unsigned long long)g.cfg.blocks_per_cu;
  const unsigned blocks = (unsigned)(want < cap ? want : cap);
  g.tag.set("k_lattice_rows", {METHOD, N, RECT, FMA}, 0b1100u);
  hipLaunchKernelGGL((k_lattice_rows<T, METHOD, N, RECT, FMA>), dim3(blocks), dim3(kLatticeBlock), lds_bytes, stream, a);
  return hipGetLastError();
}

template <typename T, int METHOD, int N>
static hipError_t launch_rows_n(const GridDesc& g, const LatticeShape& s, const void* recs, void* out, size_t lds_bytes,
                                hipStream_t stream) {
  if (g.kind == kRegular)
    return g.fma ? launch_rows_k<T, METHOD, N, false, true>(g, s, recs, out, lds_bytes, stream)
                 : launch_rows_k<T, METHOD, N, false, false>(g, s, recs, out, lds_bytes, stream);
  return g.fma ? launch_rows_k<T, METHOD, N, true, true>(g, s, recs, out, lds_bytes, stream)
               : launch_rows_k<T, METHOD, N, true, false>(g, s, recs, out, lds_bytes, stream);
}

template <typename T>
static hipError_t launch_rows_t(const GridDesc& g, const LatticeShape& s, const void* recs, void* out, size_t lds_bytes,
                                hipStream_t stream) {
  if (g.method == kLinear && g.ndims == 2) return launch_rows_n<T, kLinear, 2>(g, s, recs, out, lds_bytes, stream);
  if (g.method == kLinear && g.ndims == 3) return launch_rows_n<T, kLinear, 3>(g, s, recs, out, lds_bytes, stream);
  if (g.method == kCubic && g.ndims == 2) return launch_rows_n<T, kCubic, 2>(g, s, recs, out, lds_bytes, stream);
  if (g.method == kCubic && g.ndims == 3) return launch_rows_n<T, kCubic, 3>(g, s, recs, out, lds_bytes, stream);
  return hipErrorInvalidValue;
}

hipError_t launch_lattice_rows(const GridDesc& g, const LatticeShape& s, const void* recs, void* out, size_t lds_bytes,
                               hipStream_t stream) {
  if (s.npoints == 0) return hipSuccess;
  return g.dtype == kF64 ? launch_rows_t<double>(g, s, recs, out, lds_bytes, stream)
                         : launch_rows_t<float>(g, s, recs, out, lds_bytes, stream);
}

template <typename T>
static hipError_t launch_expand_t(const GridDesc& g, const LatticeShape& s, const unsigned char* bad, void* const* dst,
                                  size_t begin, size_t count, hipStream_t stream) {
  LatticeExpandArgs<T> a;
  a.ndims = s.ndims;
  a.bad = bad;
  a.begin = begin;
  a.count = count;
  for (int d = 0; d < kMaxDims; ++d) {
    const bool live = d < s.ndims;
    a.axes[d] = live ? static_cast<const T*>(s.axes[d]) : nullptr;
    a.dst[d] = live ? static_cast<T*>(dst[d]) : nullptr;
    a.m[d] = live ? s.m[d] : 1;
    a.rec_off[d] = live ? s.rec_off[d] : 0;
    a.subst[d] = live ? (T)g.start[d] : (T)0;
  }
  hipLaunchKernelGGL((k_lattice_expand<T>), dim3(one_pass_blocks(count, 4)), dim3(kBlock), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_lattice_expand(const GridDesc& g, const LatticeShape& s, const unsigned char* bad, void* const* dst,
                                 size_t begin, size_t count, hipStream_t stream) {
  if (count == 0) return hipSuccess;
  return g.dtype == kF64 ? launch_expand_t<double>(g, s, bad, dst, begin, count, stream)
                         : launch_expand_t<float>(g, s, bad, dst, begin, count, stream);
}

}  // namespace interpn
