// Field sets on a lattice (lattice.h, "Field sets on a lattice"): k_lattice_rows with a field loop around the row.
#include "lattice_rows.h"

namespace interpn {

template <typename T, int N>
struct LatticeFieldsRowsArgs {
  LatticeRowsArgs<T, N> r;   // vals: field 0; line_bytes: from line to line of a wave's group
  size_t field_stride;       // elements from field to field in `vals`
  size_t out_stride;         // field-major: elements from field to field; fields-last: from point to point
  unsigned nfields;
  unsigned group;            // G: fields per pass over a row
  unsigned wave_bytes;       // LDS bytes from wave to wave: G lines, then the tile (fields-last)
};

// LAST (fields-last results) is a template parameter and not a launch-uniform branch: the two stores differ in structure —
// a coalesced store per field against a tile exchange through LDS with its own index arithmetic — and as a parameter the
// field-major kernels keep k_lattice_rows' registers and carry no tile.
template <typename T, int METHOD, int N, bool RECT, bool FMA, bool LAST>
__global__ void __launch_bounds__(kLatticeBlock) k_lattice_fields_rows(const LatticeFieldsRowsArgs<T, N> fa) {
  static_assert(N == 2 || N == 3, "row kernel: N = 2, 3");
  constexpr int FP = METHOD == kLinear ? 2 : 4;
  typedef typename LatticeRec<T, METHOD, RECT>::type Rec;
  typedef LatticeDim<T, METHOD, RECT> Dim;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const LatticeRowsArgs<T, N>& a = fa.r;
  const unsigned lane = threadIdx.x & 63u;
  const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  T* lines = reinterpret_cast<T*>(smem_raw + (size_t)wave * fa.wave_bytes);
  const unsigned line_elems = a.line_bytes / (unsigned)sizeof(T);
  T* tile = lines + fa.group * line_elems;  // fields-last only
  const Rec* recs = static_cast<const Rec*>(a.recs);
  const Rec* recs_last = recs + a.rec_off[N - 1];
  const unsigned m_last = a.m[N - 1];
  const unsigned long long row_step = (unsigned long long)gridDim.x * kLatticeWaves;
  for (unsigned long long row = (unsigned long long)blockIdx.x * kLatticeWaves + wave; row < a.nrows; row += row_step) {
    // the row's records of dims 0 .. N-2: the same for every lane and every field
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
    const unsigned long long p_row = row * m_last;  // flat index of the row's first point
    for (unsigned f0 = 0; f0 < fa.nfields; f0 += fa.group) {
      const unsigned gw = fa.nfields - f0 < fa.group ? fa.nfields - f0 : fa.group;  // the last pass may be short
      // line f: r[k] of field f0 + f, dims 0 .. N-2 reduced at grid column k of the last axis (k_lattice_rows' statements)
      for (unsigned f = 0; f < gw; ++f) {
        const T* field = a.vals + (size_t)(f0 + f) * fa.field_stride;
        T* line = lines + f * line_elems;
        for (unsigned k = lane; k < (unsigned)a.n_last; k += 64u) {
          const T* col = field + base + k;
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
      }
      wave_sync();
      // the row's outputs in chunks of 64: the last axis's record once, then one node per field from that field's line
      for (unsigned j0 = 0; j0 < m_last; j0 += 64u) {
        const unsigned here = m_last - j0 < 64u ? m_last - j0 : 64u;
        const unsigned j = j0 + (lane < here ? lane : here - 1u);  // lanes behind a ragged chunk repeat its last record
        Dim last;
        last.load(recs_last[j]);
        if constexpr (!LAST) {
          T* dst = fa.r.out + (size_t)f0 * fa.out_stride + p_row + j;
          for (unsigned f = 0; f < gw; ++f) {
            const T* line = lines + f * line_elems;
            T v[FP];
#pragma unroll
            for (int i = 0; i < FP; ++i) v[i] = line[last.loc + i];
            const T res = lattice_node<FMA, T>(v, last);  // regular.rs:396-402 / multicubic/regular.rs:415-421
            if (lane < here) stream_store(dst + (size_t)f * fa.out_stride, res);
          }
        } else {
          const unsigned ts = fa.group | 1u;
          for (unsigned f = 0; f < gw; ++f) {
            const T* line = lines + f * line_elems;
            T v[FP];
#pragma unroll
            for (int i = 0; i < FP; ++i) v[i] = line[last.loc + i];
            tile[lane * ts + f] = lattice_node<FMA, T>(v, last);
          }
          wave_sync();
          // the tile's fields [f0, f0 + gw) of the chunk's `here` points, lane-contiguously: element e = (point e / gw,
          // field e % gw)
          const unsigned q = 64u / gw, r = 64u - q * gw;  // uniform: what 64 more elements add to (point, field)
          unsigned p = lane / gw;
          unsigned f = lane - p * gw;
          T* dst = fa.r.out + (size_t)(p_row + j0) * fa.out_stride + f0;
          for (unsigned k = 0; k < gw; ++k) {
            if (p < here) stream_store(dst + (size_t)p * fa.out_stride + f, tile[p * ts + f]);
            p += q;
            f += r;
            if (f >= gw) {
              f -= gw;
              ++p;
            }
          }
          wave_sync();  // the next chunk overwrites the tile
        }
      }
      wave_sync();  // the next group, or the next row, overwrites the lines
    }
  }
}

// ---------------------------------------------------------------------------
// Launchers
template <typename T, int METHOD, int N, bool RECT, bool FMA, bool LAST>
static hipError_t launch_k(const GridDesc& g, const LatticeShape& s, const void* recs, size_t field_stride, size_t nfields,
                           size_t group, void* out, size_t out_stride, size_t lds_bytes, hipStream_t stream) {
  LatticeFieldsRowsArgs<T, N> fa;
  LatticeRowsArgs<T, N>& a = fa.r;
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
  a.line_bytes = (unsigned)lattice_line_bytes((size_t)g.n[N - 1], sizeof(T));
  fa.field_stride = field_stride;
  fa.out_stride = out_stride;
  fa.nfields = (unsigned)nfields;
  fa.group = (unsigned)group;
  fa.wave_bytes = (unsigned)lattice_fields_wave_bytes((size_t)g.n[N - 1], sizeof(T), group, LAST ? kLatticeFieldsLast : kLatticeFieldMajor);
  if ((size_t)kLatticeWaves * fa.wave_bytes > lds_bytes) return hipErrorInvalidValue;  // the plan's bytes hold the waves' areas
  const unsigned long long want = (a.nrows + kLatticeWaves - 1) / kLatticeWaves;
  const unsigned long long cap = (unsigned long long)g.cfg.num_cus * (unsigned long long)g.cfg.blocks_per_cu;
  const unsigned blocks = (unsigned)(want < cap ? want : cap);
  g.tag.set("k_lattice_fields_rows", {METHOD, N, RECT, FMA, LAST}, 0b11100u);
  hipLaunchKernelGGL((k_lattice_fields_rows<T, METHOD, N, RECT, FMA, LAST>), dim3(blocks), dim3(kLatticeBlock), lds_bytes, stream, fa);
  return hipGetLastError();
}

template <typename T, int METHOD, int N, bool RECT, bool FMA>
static hipError_t launch_l(const GridDesc& g, const LatticeShape& s, const void* recs, size_t field_stride, size_t nfields,
                           size_t group, void* out, size_t out_stride, int layout, size_t lds_bytes, hipStream_t stream) {
  return layout == kLatticeFieldsLast
             ? launch_k<T, METHOD, N, RECT, FMA, true>(g, s, recs, field_stride, nfields, group, out, out_stride, lds_bytes, stream)
             : launch_k<T, METHOD, N, RECT, FMA, false>(g, s, recs, field_stride, nfields, group, out, out_stride, lds_bytes, stream);
}

template <typename T, int METHOD, int N>
static hipError_t launch_n(const GridDesc& g, const LatticeShape& s, const void* recs, size_t field_stride, size_t nfields,
                           size_t group, void* out, size_t out_stride, int layout, size_t lds_bytes, hipStream_t stream) {
  if (g.kind == kRegular)
    return g.fma ? launch_l<T, METHOD, N, false, true>(g, s, recs, field_stride, nfields, group, out, out_stride, layout, lds_bytes, stream)
                 : launch_l<T, METHOD, N, false, false>(g, s, recs, field_stride, nfields, group, out, out_stride, layout, lds_bytes, stream);
  return g.fma ? launch_l<T, METHOD, N, true, true>(g, s, recs, field_stride, nfields, group, out, out_stride, layout, lds_bytes, stream)
               : launch_l<T, METHOD, N, true, false>(g, s, recs, field_stride, nfields, group, out, out_stride, layout, lds_bytes, stream);
}

template <typename T>
static hipError_t launch_t(const GridDesc& g, const LatticeShape& s, const void* recs, size_t field_stride, size_t nfields,
                           size_t group, void* out, size_t out_stride, int layout, size_t lds_bytes, hipStream_t stream) {
#define LATTICE_FIELDS_CASE(METHOD, N) \
  if (g.method == METHOD && g.ndims == N) \
    return launch_n<T, METHOD, N>(g, s, recs, field_stride, nfields, group, out, out_stride, layout, lds_bytes, stream);
  LATTICE_FIELDS_CASE(kLinear, 2)
  LATTICE_FIELDS_CASE(kLinear, 3)
  LATTICE_FIELDS_CASE(kCubic, 2)
  LATTICE_FIELDS_CASE(kCubic, 3)
#undef LATTICE_FIELDS_CASE
  return hipErrorInvalidValue;
}

hipError_t launch_lattice_fields_rows(const GridDesc& g, const LatticeShape& s, const void* recs, size_t field_stride, size_t nfields,
                                      size_t group, void* out, size_t out_stride, int layout, size_t lds_bytes, hipStream_t stream) {
  if (group < 1 || group > nfields || group > (size_t)kLatticeFieldsCap || nfields > 0xFFFFFFFFull) return hipErrorInvalidValue;
  if (layout != kLatticeFieldMajor && layout != kLatticeFieldsLast) return hipErrorInvalidValue;
  if (layout == kLatticeFieldMajor ? out_stride < s.npoints : out_stride < nfields) return hipErrorInvalidValue;
  for (int d = 0; d < s.ndims; ++d)
    if (s.m[d] >= ((size_t)1 << 31)) return hipErrorInvalidValue;
  if (s.npoints == 0) return hipSuccess;
  return g.dtype == kF64 ? launch_t<double>(g, s, recs, field_stride, nfields, group, out, out_stride, layout, lds_bytes, stream)
                         : launch_t<float>(g, s, recs, field_stride, nfields, group, out, out_stride, layout, lds_bytes, stream);
}

}  // namespace interpn
