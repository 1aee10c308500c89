// Host side of the tiled multicubic table (cubic_brick.h): its geometry, its builder, and the launcher of k_cubic_brick,
// which sets the kernel's own arguments (binned and gated forms, per-cell records) and goes through cubic_cell_launch.h.
#include "cubic_cell_launch.h"

namespace interpn {

void cubic_tile_geometry(const GridDesc& g, int si, int sj, unsigned nb[2], size_t* bytes) {
  nb[0] = (unsigned)((g.n[0] - 4) / si + 2);
  nb[1] = (unsigned)((g.n[1] - 4) / sj + 2);
  size_t planes = 1;
  for (int d = 2; d < g.ndims; ++d) planes *= (size_t)g.n[d];
  *bytes = planes * nb[0] * nb[1] * 16 * (g.dtype == kF64 ? 8 : 4);
}

hipError_t build_cubic_tiles(const GridDesc& g, void* tiles, hipStream_t stream) {
  size_t planes = 1;
  for (int d = 2; d < g.ndims; ++d) planes *= (size_t)g.n[d];
  const size_t elems = planes * g.brick_nb[0] * g.brick_nb[1] * 16;
  size_t blocks = (elems + kBlock - 1) / kBlock;
  if (blocks > 65535) blocks = 65535;
  if (g.dtype == kF64)
    hipLaunchKernelGGL(k_build_cubic_tiles<double>, dim3((unsigned)blocks), dim3(kBlock), 0, stream,
                       static_cast<const double*>(g.vals), static_cast<double*>(tiles), planes, g.n[0], g.n[1],
                       g.brick_step[0], g.brick_step[1], g.brick_nb[0], g.brick_nb[1]);
  else
    hipLaunchKernelGGL(k_build_cubic_tiles<float>, dim3((unsigned)blocks), dim3(kBlock), 0, stream,
                       static_cast<const float*>(g.vals), static_cast<float*>(tiles), planes, g.n[0], g.n[1],
                       g.brick_step[0], g.brick_step[1], g.brick_nb[0], g.brick_nb[1]);
  return hipGetLastError();
}

struct CubicBrickKernel {
  static constexpr const char* name = "k_cubic_brick";
  template <typename T, int N> using Args = CubicBrickArgs<T, N>;
  template <typename T, int N, bool RECT, bool FMA, int SI, int SJ>
  static auto kernel() { return &k_cubic_brick<T, N, RECT, FMA, SI, SJ>; }
};

template <typename T, int N>
static hipError_t launch_n(const GridDesc& g, const T* const* obs, T* out, size_t npts, unsigned long long* first_bad,
                           hipStream_t stream, const unsigned* scatter, size_t index_base) {
  CubicBrickArgs<T, N> a;
  a.out = out;
  a.scatter = scatter;
  a.index_base = index_base;
  for (int d = 0; d < N; ++d) {
    a.obs[d] = obs[d];
    a.crec[d] = (g.kind == kRectilinear && g.axis_crec_bytes)
                    ? reinterpret_cast<const CubicCellRecord<T>*>(static_cast<const unsigned char*>(g.axis_image) + g.axis_crec_off[d]) : nullptr;
  }
  unsigned blocks = grid_blocks(npts, 1, g.cfg);
  a.gate = scatter ? nullptr : g.launch_gate;
  a.eighth = 0;
  if (scatter && g.cfg.deal && blocks >= 64) {
    blocks &= ~7u;  // eight equal XCD shares; the grid-stride loop covers what the rounding drops
    a.eighth = ((npts + 7) / 8 + kBlock - 1) / kBlock * kBlock;
  }
  return cubic_cell_launch<CubicBrickKernel, T, N>(g, a, npts, first_bad, blocks, stream);
}

template <typename T>
hipError_t launch_cubic_brick(const GridDesc& g, const T* const* obs, T* out, size_t npts,
                              unsigned long long* first_bad, hipStream_t stream, const unsigned* scatter, size_t index_base) {
  switch (g.ndims) {
    case 2: return launch_n<T, 2>(g, obs, out, npts, first_bad, stream, scatter, index_base);
    case 3: return launch_n<T, 3>(g, obs, out, npts, first_bad, stream, scatter, index_base);
    case 4: return launch_n<T, 4>(g, obs, out, npts, first_bad, stream, scatter, index_base);
    default: return hipErrorInvalidValue;
  }
}

template hipError_t launch_cubic_brick<double>(const GridDesc&, const double* const*, double*, size_t, unsigned long long*, hipStream_t,
                                               const unsigned*, size_t);
template hipError_t launch_cubic_brick<float>(const GridDesc&, const float* const*, float*, size_t, unsigned long long*, hipStream_t,
                                              const unsigned*, size_t);

}  // namespace interpn
