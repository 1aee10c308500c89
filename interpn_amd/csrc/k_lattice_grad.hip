// Gradients on a lattice (lattice_grad.h): the launcher of k_lattice_grad_rows, 32 instantiations
// ({f64, f32} x {multilinear, multicubic} x N = 2, 3 x {regular, rectilinear} x {fma, no fma}).
#include "lattice_grad.h"

namespace interpn {

template <typename T, int METHOD, int N, bool RECT, bool FMA>
static hipError_t launch_grad_rows_k(const GridDesc& g, const LatticeShape& s, const void* recs, void* out, void* const* grad,
                                     size_t lds_bytes, hipStream_t stream) {
  LatticeGradRowsArgs<T, N> ga;
  LatticeRowsArgs<T, N>& a = ga.r;
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
    ga.grad[d] = static_cast<T*>(grad[d]);
    ga.grid[d] = RECT ? static_cast<const T*>(g.grid[d]) : nullptr;
    ga.step[d] = (T)g.step[d];
  }
  a.n_last = g.n[N - 1];
  a.line_bytes = 0;
  ga.wave_bytes = (unsigned)(lds_bytes / kLatticeWaves);
  const unsigned long long want = (a.nrows + kLatticeWaves - 1) / kLatticeWaves;
  const unsigned long long cap = (unsigned long long)g.cfg.num_cus * (unsigned long long)g.cfg.blocks_per_cu;
  const unsigned blocks = (unsigned)(want < cap ? want : cap);
  g.tag.set("k_lattice_grad_rows", {METHOD, N, RECT, FMA}, 0b1100u);
  hipLaunchKernelGGL((k_lattice_grad_rows<T, METHOD, N, RECT, FMA>), dim3(blocks), dim3(kLatticeBlock), lds_bytes, stream, ga);
  return hipGetLastError();
}

template <typename T, int METHOD, int N>
static hipError_t launch_grad_rows_n(const GridDesc& g, const LatticeShape& s, const void* recs, void* out, void* const* grad,
                                     size_t lds_bytes, hipStream_t stream) {
  if (g.kind == kRegular)
    return g.fma ? launch_grad_rows_k<T, METHOD, N, false, true>(g, s, recs, out, grad, lds_bytes, stream)
                 : launch_grad_rows_k<T, METHOD, N, false, false>(g, s, recs, out, grad, lds_bytes, stream);
  return g.fma ? launch_grad_rows_k<T, METHOD, N, true, true>(g, s, recs, out, grad, lds_bytes, stream)
               : launch_grad_rows_k<T, METHOD, N, true, false>(g, s, recs, out, grad, lds_bytes, stream);
}

template <typename T>
static hipError_t launch_grad_rows_t(const GridDesc& g, const LatticeShape& s, const void* recs, void* out, void* const* grad,
                                     size_t lds_bytes, hipStream_t stream) {
  if (g.method == kLinear && g.ndims == 2) return launch_grad_rows_n<T, kLinear, 2>(g, s, recs, out, grad, lds_bytes, stream);
  if (g.method == kLinear && g.ndims == 3) return launch_grad_rows_n<T, kLinear, 3>(g, s, recs, out, grad, lds_bytes, stream);
  if (g.method == kCubic && g.ndims == 2) return launch_grad_rows_n<T, kCubic, 2>(g, s, recs, out, grad, lds_bytes, stream);
  if (g.method == kCubic && g.ndims == 3) return launch_grad_rows_n<T, kCubic, 3>(g, s, recs, out, grad, lds_bytes, stream);
  return hipErrorInvalidValue;
}

hipError_t launch_lattice_grad_rows(const GridDesc& g, const LatticeShape& s, const void* recs, void* out, void* const* grad,
                                    size_t lds_bytes, hipStream_t stream) {
  if (s.npoints == 0) return hipSuccess;
  return g.dtype == kF64 ? launch_grad_rows_t<double>(g, s, recs, out, grad, lds_bytes, stream)
                         : launch_grad_rows_t<float>(g, s, recs, out, grad, lds_bytes, stream);
}

}  // namespace interpn
