// interpn::one_dim (src/one_dim/*.rs): Linear1D, LinearHoldLast1D, Left1D, Right1D, Nearest1D on a RegularGrid1D or a
// RectilinearGrid1D.  Not multilinear with N = 1: the cell's coordinates and the result have formulas of their own.
//
// Per point (Interp1D::eval_one through Grid1D::at, one_dim/mod.rs:121-137 and :171-186):
//   regular      extrap: loc > stop -> high, loc < start -> low, else inside (NaN: inside)     one_dim/mod.rs:100-104
//                i = floor((loc - start) / step) as isize, clamped to [0, n-2]; the cast fails ("Unrepresentable
//                number") for NaN, +-inf and |i| >= 2^63                                          one_dim/mod.rs:107-113
//                x0 = start + step * T(i) (two roundings), x1 = x0 + step                          one_dim/mod.rs:124-126
//   rectilinear  i = clamp(partition_point(g < loc) - 1, 0, n-2); extrap: loc < g[0] -> low, loc > g[n-1] -> high
//                (note the order: the reverse of the regular grid's)                               one_dim/mod.rs:157-166
//   Left1D       y1 if high, else y0                                                               one_dim/hold.rs:33-36
//   Right1D      y0 if low, else y1                                                                one_dim/hold.rs:68-71
//   Nearest1D    y0 if |loc - x1| >= |loc - x0| else y1 (a tie goes left, NaN right)               one_dim/hold.rs:98-104
//   Linear1D     slope = (y1 - y0) / (x1 - x0); y0 + slope * (loc - x0), fused under `fma`        one_dim/linear.rs:28-34
//   LinearHoldLast1D  inside: Linear1D (fused site one_dim/linear.rs:76); low: y0, high: y1 of the clamped cell
//                                                                                                  one_dim/linear.rs:68-81
// Everything a point needs that depends on its cell alone is computed ONCE per cell at creation, on the device and with
// the reference's own operations (k_build_one_dim): x0, x1, the slope.  IEEE subtraction and division are correctly
// rounded, so a per-cell constant has the bits the reference computes per point.  Records (T = element type):
//   Linear1D / LinearHoldLast1D  {x0, y0, slope, y1}   Nearest1D {x0, x1, y0, y1}   Left1D / Right1D {y0, y1}
// A point then costs its 2*sizeof(T) bytes of streams, the cell search and one record read.  While the table (records,
// plus the coordinates and the bucket table of a rectilinear axis) fits an LDS budget (60 KiB by default, option
// "axis_lds_kb") every workgroup of a persistent grid stages it once; larger tables are read through the caches.
//
// The regular cell index without a division: floor_quotient_fast (interpn_device.h) gives floor(RN(a0 / step)) from
// qt = RN(a0 * RN(1 / step)) when qt is far enough from an integer and |qt| < 2^31 (f32: 2^20), which also settles the
// isize check; the host admits the step for it (2^-128 <= step <= 2^128, f32 2^-16 .. 2^16).  Other lanes (exact knots,
// points far outside, negative / zero / NaN steps) take the IEEE division.
#include "interpn_kernels.h"

namespace interpn {

template <typename T, int W>
struct __attribute__((aligned(W * sizeof(T)))) OdRec {
  T v[W];
};

// record width in elements per method
template <int OP> struct OdWidth { static constexpr int value = (OP == kLeft1D || OP == kRight1D) ? 2 : 4; };

template <typename T>
struct OneDimArgs {
  const unsigned char* table;  // records [+ coordinates at g_off + bucket table at tab_off]
  const T* obs;
  T* out;
  size_t npts;
  unsigned long long* first_bad;
  size_t g_off, tab_off;
  unsigned stage_bytes;  // bytes of `table` staged into LDS (LDS kernels)
  int n, M;
  T lo, hi;              // regular: start, stop; rectilinear: g[0], g[n-1]
  T start, step, rstep;  // regular
  T g0, scale;           // rectilinear bucket table
  int fast;              // regular: the step admits floor_quotient_fast
};

__device__ __forceinline__ double od_abs(double x) { return __builtin_fabs(x); }
__device__ __forceinline__ float od_abs(float x) { return __builtin_fabsf(x); }

// One point.  false: the regular grid's isize cast fails ("Unrepresentable number"); *y is then not written.
template <typename T, int OP, int KIND, bool FMA>
__device__ __forceinline__ bool od_eval(const OneDimArgs<T>& a, const unsigned char* base, T x, T* y) {
  int ext;  // 0 inside, 1 outside low, 2 outside high
  int i;
  if constexpr (KIND == kRegular) {
    ext = x > a.hi ? 2 : (x < a.lo ? 1 : 0);  // one_dim/mod.rs:100-104
    const T a0 = x - a.start;
    T floc;
    const bool fast = a.fast && floor_quotient_fast(a0, a.rstep, &floc);
    if (!fast) {
      floc = dev_floor<T>(a0 / a.step);  // one_dim/mod.rs:107
      // <isize as NumCast>::from: Some iff -2^63 <= f < 2^63 (NaN: None)      one_dim/mod.rs:110-111
      if (!((floc >= (T)-9223372036854775808.0) && (floc < (T)9223372036854775808.0))) return false;
    }
    i = clamp_loc<T>(floc, a.n - 2);  // .max(0).min(n - 2), one_dim/mod.rs:112-113
  } else {
    Axis<T> ax;
    ax.g = reinterpret_cast<const T*>(base + a.g_off);
    ax.tab = reinterpret_cast<const unsigned*>(base + a.tab_off);
    ax.n = a.n;
    ax.M = a.M;
    ax.g0 = a.g0;
    ax.scale = a.scale;
    int l = axis_partition_point<T>(ax, x) - 1;  // one_dim/mod.rs:158-159 (NaN: 0 -> cell 0)
    l = l > 0 ? l : 0;
    i = l < a.n - 2 ? l : a.n - 2;
    ext = x < a.lo ? 1 : (x > a.hi ? 2 : 0);  // one_dim/mod.rs:161-165
  }
  constexpr int W = OdWidth<OP>::value;
  const OdRec<T, W> r = reinterpret_cast<const OdRec<T, W>*>(base)[i];
  if constexpr (OP == kLeft1D) {
    *y = ext == 2 ? r.v[1] : r.v[0];
  } else if constexpr (OP == kRight1D) {
    *y = ext == 1 ? r.v[0] : r.v[1];
  } else if constexpr (OP == kNearest1D) {
    const T dx0 = od_abs(x - r.v[0]);
    const T dx1 = od_abs(x - r.v[1]);
    *y = dx1 >= dx0 ? r.v[2] : r.v[3];
  } else {
    const T v = mul_add<FMA>(r.v[2], x - r.v[0], r.v[1]);  // slope.mul_add(dx, y0), one_dim/linear.rs:34 / :76
    if constexpr (OP == kLinear1D) *y = v;
    else *y = ext == 0 ? v : (ext == 1 ? r.v[1] : r.v[3]);
  }
  return true;
}

__device__ __forceinline__ void od_fail(unsigned long long* first_bad, size_t i) {
  atomicMin(first_bad, (unsigned long long)i);
}

// PPL points per lane (2: 2*sizeof(T)-byte streams, obs and out aligned to that).  LDS: the workgroup stages the first
// stage_bytes of the table and runs a grid-stride loop (a persistent grid); otherwise one pass reading the table
// through the caches.
template <typename T, int OP, int KIND, bool FMA, bool LDS, int PPL>
__global__ void __launch_bounds__(kBlock) k_one_dim(const OneDimArgs<T> a) {
  typedef T T2 __attribute__((ext_vector_type(2)));
  extern __shared__ __attribute__((aligned(16))) unsigned char od_lds[];
  const unsigned char* base = a.table;
  if constexpr (LDS) {
    typedef unsigned U4 __attribute__((ext_vector_type(4)));
    for (unsigned o = threadIdx.x * 16u; o < a.stage_bytes; o += kBlock * 16u)
      *reinterpret_cast<U4*>(od_lds + o) = *reinterpret_cast<const U4*>(a.table + o);
    __syncthreads();
    base = od_lds;
  }
  const size_t nslots = (a.npts + PPL - 1) / PPL;
  const size_t stride = (size_t)gridDim.x * kBlock;
  for (size_t s = (size_t)blockIdx.x * kBlock + threadIdx.x; s < nslots; s += stride) {
    const size_t i0 = s * PPL;
    if (PPL == 2 && i0 + 1 < a.npts) {
      const T2 x = stream_load(reinterpret_cast<const T2*>(a.obs + i0));
      T2 r;
      T y0, y1;
      const bool ok0 = od_eval<T, OP, KIND, FMA>(a, base, x.x, &y0);
      const bool ok1 = od_eval<T, OP, KIND, FMA>(a, base, x.y, &y1);
      if (ok0 && ok1) {
        r.x = y0;
        r.y = y1;
        stream_store(reinterpret_cast<T2*>(a.out + i0), r);
      } else {
        if (ok0) stream_store(a.out + i0, y0);
        else od_fail(a.first_bad, i0);
        if (ok1) stream_store(a.out + i0 + 1, y1);
        else od_fail(a.first_bad, i0 + 1);
      }
    } else {
      T y;
      if (od_eval<T, OP, KIND, FMA>(a, base, stream_load(a.obs + i0), &y)) stream_store(a.out + i0, y);
      else od_fail(a.first_bad, i0);
    }
  }
}

// Cell records, one thread per cell, with the reference's operations in T (no contraction: -ffp-contract=off).
// FORM 0: {x0, y0, slope, y1}; 1: {x0, x1, y0, y1}; 2: {y0, y1}.
template <typename T, int FORM, int KIND>
__global__ void __launch_bounds__(kBlock) k_build_one_dim(const T* __restrict__ vals, const T* __restrict__ g, int n, T start,
                                                          T step, unsigned char* __restrict__ table) {
  // size_t: with up to 2^31 - 257 values, i + stride can pass 2^31
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i + 1 < (size_t)n; i += (size_t)gridDim.x * kBlock) {
    T x0, x1;
    if constexpr (KIND == kRegular) {
      const T ti = (T)(int)i;  // <T as NumCast>::from(i): rounds once i > 2^24 in f32 (i < 2^31)
      x0 = start + step * ti;  // one_dim/mod.rs:124-125
      x1 = x0 + step;          // one_dim/mod.rs:126
    } else {
      x0 = g[i];               // one_dim/mod.rs:176
      x1 = g[i + 1];
    }
    const T y0 = vals[i], y1 = vals[i + 1];
    if constexpr (FORM == 2) {
      OdRec<T, 2> r;
      r.v[0] = y0;
      r.v[1] = y1;
      reinterpret_cast<OdRec<T, 2>*>(table)[i] = r;
    } else {
      OdRec<T, 4> r;
      if constexpr (FORM == 1) {
        r.v[0] = x0;
        r.v[1] = x1;
        r.v[2] = y0;
        r.v[3] = y1;
      } else {
        r.v[0] = x0;
        r.v[1] = y0;
        r.v[2] = (y1 - y0) / (x1 - x0);  // one_dim/linear.rs:28 / :70
        r.v[3] = y1;
      }
      reinterpret_cast<OdRec<T, 4>*>(table)[i] = r;
    }
  }
}

static int od_form(int method) { return method == kNearest1D ? 1 : ((method == kLeft1D || method == kRight1D) ? 2 : 0); }

size_t one_dim_record_bytes(const GridDesc& g) {
  const size_t elem = g.dtype == kF64 ? 8 : 4;
  return (size_t)(g.n[0] - 1) * elem * (od_form(g.method) == 2 ? 2 : 4);
}

template <typename T>
static hipError_t build_table_t(const GridDesc& g, void* table, hipStream_t stream) {
  const int n = g.n[0];
  const unsigned blocks = (unsigned)std::min<size_t>(((size_t)n + kBlock - 2) / kBlock, (size_t)1 << 20);
  const T* vals = static_cast<const T*>(g.vals);
  const T* gr = static_cast<const T*>(g.grid[0]);
  unsigned char* t = static_cast<unsigned char*>(table);
  const T start = (T)g.od_start, step = (T)g.od_step;
#define BUILD(FORM, KIND) hipLaunchKernelGGL((k_build_one_dim<T, FORM, KIND>), dim3(blocks), dim3(kBlock), 0, stream, vals, gr, n, start, step, t)
  const int form = od_form(g.method);
  if (g.kind == kRegular) {
    if (form == 0) BUILD(0, kRegular); else if (form == 1) BUILD(1, kRegular); else BUILD(2, kRegular);
  } else {
    if (form == 0) BUILD(0, kRectilinear); else if (form == 1) BUILD(1, kRectilinear); else BUILD(2, kRectilinear);
  }
#undef BUILD
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || g.kind != kRectilinear) return e;
  // the coordinates and (sorted finite axes) the bucket table behind the records, so that one copy stages all of it
  T* gcopy = reinterpret_cast<T*>(t + g.od_g_off);
  e = hipMemcpyAsync(gcopy, gr, (size_t)n * sizeof(T), hipMemcpyDeviceToDevice, stream);
  if (e == hipSuccess && g.od_M > 0)
    e = build_buckets<T>(gcopy, n, g.od_M, (T)g.od_g0, (T)g.od_scale, reinterpret_cast<unsigned*>(t + g.od_tab_off), stream);
  return e;
}

hipError_t build_one_dim_table(const GridDesc& g, void* table, hipStream_t stream) {
  return g.dtype == kF64 ? build_table_t<double>(g, table, stream) : build_table_t<float>(g, table, stream);
}

template <typename T, int OP, int KIND, bool FMA>
static void od_go(const GridDesc& g, const OneDimArgs<T>& a, bool lds, int ppl, unsigned blocks, hipStream_t stream) {
  const size_t shm = lds ? a.stage_bytes : 0;
#define GO(L, P)                                                                                                     \
  do {                                                                                                               \
    g.tag.set("k_one_dim", {OP, KIND, FMA, L, P}, 0b01100u);                                                         \
    hipLaunchKernelGGL((k_one_dim<T, OP, KIND, FMA, L, P>), dim3(blocks), dim3(kBlock), shm, stream, a);            \
  } while (0)
  if (lds) { if (ppl == 2) GO(true, 2); else GO(true, 1); }
  else { if (ppl == 2) GO(false, 2); else GO(false, 1); }
#undef GO
}

template <typename T, int KIND>
static void od_dispatch(const GridDesc& g, const OneDimArgs<T>& a, bool lds, int ppl, unsigned blocks, hipStream_t stream) {
  switch (g.method) {
    case kLinear1D:
      if (g.fma) od_go<T, kLinear1D, KIND, true>(g, a, lds, ppl, blocks, stream);
      else od_go<T, kLinear1D, KIND, false>(g, a, lds, ppl, blocks, stream);
      break;
    case kLinearHoldLast1D:
      if (g.fma) od_go<T, kLinearHoldLast1D, KIND, true>(g, a, lds, ppl, blocks, stream);
      else od_go<T, kLinearHoldLast1D, KIND, false>(g, a, lds, ppl, blocks, stream);
      break;
    // the hold and nearest methods have no fused site: one instantiation serves both flavours
    case kLeft1D: od_go<T, kLeft1D, KIND, false>(g, a, lds, ppl, blocks, stream); break;
    case kRight1D: od_go<T, kRight1D, KIND, false>(g, a, lds, ppl, blocks, stream); break;
    default: od_go<T, kNearest1D, KIND, false>(g, a, lds, ppl, blocks, stream); break;
  }
}

template <typename T>
static hipError_t launch_t(const GridDesc& g, const T* obs, T* out, size_t npts, unsigned long long* first_bad,
                           hipStream_t stream) {
  OneDimArgs<T> a;
  a.table = static_cast<const unsigned char*>(g.bricks);
  a.obs = obs;
  a.out = out;
  a.npts = npts;
  a.first_bad = first_bad;
  a.g_off = g.od_g_off;
  a.tab_off = g.od_tab_off;
  a.n = g.n[0];
  a.M = g.od_M;
  a.start = (T)g.od_start;
  a.step = (T)g.od_step;
  a.rstep = (T)g.od_rstep;
  a.fast = g.od_fast;
  a.g0 = (T)g.od_g0;
  a.scale = (T)g.od_scale;
  a.lo = g.kind == kRegular ? (T)g.od_start : (T)g.bound_lo[0];
  a.hi = g.kind == kRegular ? (T)g.od_stop : (T)g.bound_hi[0];
  const size_t stage = (g.od_table_bytes + 15) & ~(size_t)15;
  const size_t budget = g.cfg.axis_lds_kb >= 0 ? (size_t)g.cfg.axis_lds_kb * 1024 : thresholds(g.cfg).axis_lds_wide;
  const bool lds = stage <= budget && stage <= (size_t)g.cfg.lds_per_wg;
  a.stage_bytes = (unsigned)(lds ? stage : 0);
  const bool aligned = (reinterpret_cast<uintptr_t>(out) % (2 * sizeof(T))) == 0 &&
                       (reinterpret_cast<uintptr_t>(obs) % (2 * sizeof(T))) == 0;
  const int ppl = (aligned && g.cfg.ppl != 1) ? 2 : 1;
  unsigned blocks = one_pass_blocks(npts, ppl);
  if (lds) {
    // persistent: as many workgroups as the LDS lets a CU hold (at most blocks_per_cu), two rounds of them
    size_t per_cu = stage ? (size_t)g.cfg.lds_per_cu / stage : (size_t)g.cfg.blocks_per_cu;
    per_cu = std::max<size_t>(1, std::min<size_t>(per_cu, (size_t)g.cfg.blocks_per_cu));
    blocks = (unsigned)std::min<size_t>(blocks, (size_t)g.cfg.num_cus * per_cu * 2);
  }
  if (g.kind == kRegular) od_dispatch<T, kRegular>(g, a, lds, ppl, blocks, stream);
  else od_dispatch<T, kRectilinear>(g, a, lds, ppl, blocks, stream);
  return hipGetLastError();
}

hipError_t launch_one_dim(const GridDesc& g, const void* obs, void* out, size_t npts, unsigned long long* first_bad,
                          hipStream_t stream) {
  if (npts == 0) return hipSuccess;
  if (g.dtype == kF64)
    return launch_t<double>(g, static_cast<const double*>(obs), static_cast<double*>(out), npts, first_bad, stream);
  return launch_t<float>(g, static_cast<const float*>(obs), static_cast<float*>(out), npts, first_bad, stream);
}

}  // namespace interpn
