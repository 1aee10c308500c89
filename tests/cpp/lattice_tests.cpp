// `interp_lattice` of the C++ mirror (include/interpn_hip.hpp -> interpn_hip_eval_lattice_host -> k_lattice.hip) against
// `interp` on the expanded points: the four multilinear / multicubic mirrors in 2 and 3 dimensions (the fused row
// kernel where the automatic rule takes it, else the expanded path), the nearest-neighbour mirrors and a 4-D grid
// (always expanded), equality bit for bit; then the error contract.
//
// Build (tests/test_cpp_lattice.py does this):
//   g++ -std=c++17 -O1 -Iinclude tests/cpp/lattice_tests.cpp -Linterpn_amd -linterpn_hip
//       -Wl,-rpath,$PWD/interpn_amd -o lattice_tests
// Prints one line per test and "ALL PASSED" / exit code 0 when every assertion held.  Needs a GPU.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>

#include "interpn_hip.hpp"

using namespace interpn_hip;
using utils::linspace;

static int g_failures = 0;
#define EXPECT(cond)                                                                     \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      if (g_failures < 20) std::printf("  FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failures;                                                                      \
    }                                                                                    \
  } while (0)

static void run(const char* name, const std::function<void()>& f) {
  const int before = g_failures;
  f();
  std::printf("%s %s\n", g_failures == before ? "PASS" : "FAIL", name);
}

struct Rng {  // splitmix64, uniform [0, 1)
  std::uint64_t s;
  double uniform() {
    std::uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
  }
};

template <class T>
static bool same_bits(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0;
}

// Unsorted coordinates over the grid's extent widened by a tenth on each side, exact knots among them.
template <class T>
static std::vector<T> axis_vector(const std::vector<T>& grid, std::size_t m, Rng& rng) {
  const double lo = (double)grid.front(), hi = (double)grid.back(), w = 0.1 * (hi - lo);
  std::vector<T> x(m);
  for (auto& v : x) v = (T)(lo - w + (hi - lo + 2 * w) * rng.uniform());
  if (m > 3) { x[1] = grid.front(); x[2] = grid.back(); x[3] = grid[grid.size() / 2]; }
  return x;
}

// SoA expansion in C order.
template <class T, std::size_t N>
static std::array<std::vector<T>, N> expand(const std::array<std::vector<T>, N>& axes) {
  std::size_t total = 1;
  for (const auto& a : axes) total *= a.size();
  std::array<std::vector<T>, N> pts;
  for (auto& p : pts) p.resize(total);
  for (std::size_t i = 0; i < total; ++i) {
    std::size_t rem = i;
    for (std::size_t d = N; d-- > 0;) {
      pts[d][i] = axes[d][rem % axes[d].size()];
      rem /= axes[d].size();
    }
  }
  return pts;
}

template <class T, std::size_t N>
static std::array<Slice<T>, N> views(const std::array<std::vector<T>, N>& v) {
  std::array<Slice<T>, N> s;
  for (std::size_t d = 0; d < N; ++d) s[d] = Slice<T>(v[d]);
  return s;
}

// One interpolator: interp_lattice == interp on the expanded points.
template <class T, std::size_t N, class Interp>
static void compare(const Interp& it, const std::array<std::vector<T>, N>& grids, const std::array<std::size_t, N>& lens, Rng& rng) {
  std::array<std::vector<T>, N> axes;
  std::size_t total = 1;
  for (std::size_t d = 0; d < N; ++d) {
    axes[d] = axis_vector<T>(grids[d], lens[d], rng);
    total *= lens[d];
  }
  const auto pts = expand<T, N>(axes);
  std::vector<T> want(total, (T)-1), got(total, (T)-2);
  EXPECT(it.interp(views<T, N>(pts), want).is_ok());
  EXPECT(it.interp_lattice(views<T, N>(axes), got).is_ok());
  EXPECT(same_bits(got, want));
}

template <class T, std::size_t N>
static void all_mirrors(const std::array<std::size_t, N>& dims, const std::array<std::size_t, N>& lens, std::uint64_t seed) {
  Rng rng{seed};
  std::array<std::vector<T>, N> grids, jittered;
  std::array<T, N> starts, steps;
  std::size_t nvals = 1;
  for (std::size_t d = 0; d < N; ++d) {
    grids[d] = linspace<T>((T)-1, (T)(1 + d), dims[d]);
    starts[d] = grids[d][0];
    steps[d] = grids[d][1] - grids[d][0];
    jittered[d] = grids[d];
    for (std::size_t i = 1; i + 1 < dims[d]; ++i) jittered[d][i] += (T)(0.3 * (rng.uniform() - 0.5)) * steps[d];
    nvals *= dims[d];
  }
  std::vector<T> vals(nvals);
  for (auto& v : vals) v = (T)(2 * rng.uniform() - 1);
  compare<T, N>(MultilinearRegular<T, N>::new_(dims, starts, steps, vals).unwrap(), grids, lens, rng);
  compare<T, N>(MultilinearRectilinear<T, N>::new_(views<T, N>(jittered), vals).unwrap(), jittered, lens, rng);
  for (bool linearize : {false, true}) {
    compare<T, N>(MulticubicRegular<T, N>::new_(dims, starts, steps, vals, linearize).unwrap(), grids, lens, rng);
    compare<T, N>(MulticubicRectilinear<T, N>::new_(views<T, N>(jittered), vals, linearize).unwrap(), jittered, lens, rng);
  }
  compare<T, N>(NearestRegular<T, N>::new_(dims, starts, steps, vals).unwrap(), grids, lens, rng);
  compare<T, N>(NearestRectilinear<T, N>::new_(views<T, N>(jittered), vals).unwrap(), jittered, lens, rng);
}

static void error_contract() {
  const std::array<std::size_t, 2> dims{5, 6};
  const std::array<double, 2> starts{0.0, 0.0}, steps{1.0, 1.0};
  std::vector<double> vals(30);
  for (std::size_t i = 0; i < vals.size(); ++i) vals[i] = (double)(i * i % 7);
  auto it = MultilinearRegular<double, 2>::new_(dims, starts, steps, vals).unwrap();
  std::array<std::vector<double>, 2> axes{std::vector<double>{0.5, 1.5, 2.5}, std::vector<double>{0.25, 4.75, 1.0, 3.5}};
  std::vector<double> out(12, -1.0), shorter(11, -1.0);
  auto r = it.interp_lattice(views<double, 2>(axes), shorter);
  EXPECT(r.is_err() && std::strcmp(r.err(), "Dimension mismatch") == 0);
  EXPECT(it.interp_lattice(views<double, 2>(axes), out).is_ok());
  const auto pts = expand<double, 2>(axes);
  std::vector<double> want(12, -2.0);
  EXPECT(it.interp(views<double, 2>(pts), want).is_ok() && same_bits(out, want));
  // a NaN at position 2 of axis 0 fails the lattice from point 2 * 4 on: exactly the prefix is written
  axes[0][2] = NAN;
  std::vector<double> part(12, -1.0);
  auto u = it.interp_lattice(views<double, 2>(axes), part);
  EXPECT(u.is_err() && std::strcmp(u.err(), "Unrepresentable coordinate value") == 0);
  for (std::size_t i = 0; i < 12; ++i) EXPECT(i < 8 ? part[i] == want[i] : part[i] == -1.0);
  // an empty axis: no points, nothing written
  axes[1].clear();
  std::vector<double> none;
  EXPECT(it.interp_lattice(views<double, 2>(axes), none).is_ok());
  // one_dim handles have no lattice form
  const auto g = RegularGrid1D<double>::new_(0.0, 1.0, vals).unwrap();
  auto lin = Linear1D<RegularGrid1D<double>>::new_(g).unwrap();
  std::array<std::vector<double>, 1> a1{std::vector<double>{0.5, 1.5}};
  std::vector<double> o1(2);
  EXPECT(lin.interp_lattice(views<double, 1>(a1), o1).status() == INTERPN_HIP_ERR_UNSUPPORTED);
}

int main() {
  if (interpn_hip_device_count() < 1) {
    std::printf("no HIP device: the library has no CPU path\n");
    return 2;
  }
  run("interp_lattice 2-D f64 (fused)", [] { all_mirrors<double, 2>({9, 13}, {1100, 37}, 1); });
  run("interp_lattice 3-D f64 (fused)", [] { all_mirrors<double, 3>({7, 9, 8}, {33, 35, 70}, 2); });
  run("interp_lattice 3-D f32 (fused)", [] { all_mirrors<float, 3>({7, 9, 8}, {33, 35, 70}, 3); });
  run("interp_lattice 2-D f32 (few rows: expanded)", [] { all_mirrors<float, 2>({9, 13}, {5, 37}, 4); });
  run("interp_lattice 4-D f64 (expanded)", [] { all_mirrors<double, 4>({5, 4, 6, 7}, {4, 3, 5, 6}, 5); });
  run("interp_lattice error contract", error_contract);
  if (g_failures == 0) std::printf("ALL PASSED\n");
  return g_failures == 0 ? 0 : 1;
}
