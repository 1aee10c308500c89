// The reference crate's one_dim unit tests re-created against the C++ mirror (include/interpn_hip.hpp ->
// C ABI -> k_one_dim.hip): test_hold_1d (one_dim/hold.rs:118-179) and test_linear_1d (one_dim/linear.rs:96-179), plus
// the error strings of one_dim/mod.rs.  The reference draws its points from `randn` (src/testing.rs:18), which is a
// uniform [0, 1) stream despite its name; each test runs once on a seeded uniform stream as the reference does and
// once on a seeded normal stream (Box-Muller), which puts more points far outside the grid.
//
// Build (tests/test_cpp_one_dim.py does this):
//   g++ -std=c++17 -O1 -Iinclude tests/cpp/one_dim_tests.cpp -Linterpn_amd -linterpn_hip
//       -Wl,-rpath,$PWD/interpn_amd -o one_dim_tests
// Prints one line per test and "ALL PASSED" / exit code 0 when every assertion held.  Needs a GPU.
#include <algorithm>
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

// seeded streams: uniform [0, 1) (splitmix64) and standard normal (Box-Muller on it)
struct Rng {
  std::uint64_t s;
  bool normal;
  double uniform() {
    std::uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
  }
  double next() {
    if (!normal) return uniform();
    const double u1 = 1.0 - uniform(), u2 = uniform();
    return std::sqrt(-2.0 * std::log(u1)) * std::cos(6.283185307179586 * u2);
  }
  std::vector<double> randn(std::size_t n) {
    std::vector<double> v(n);
    for (auto& x : v) x = next();
    return v;
  }
};

// partition_point(|v| v < &loc) on a sorted slice (the tests' own cell rule)
static std::size_t cell_of(const std::vector<double>& xs, double loc) {
  const std::size_t p = (std::size_t)(std::lower_bound(xs.begin(), xs.end(), loc) - xs.begin());
  const long long j = std::max<long long>((long long)p - 1, 0);
  return std::min<std::size_t>((std::size_t)j, xs.size() - 2);
}

static void hold_1d(bool normal) {  // one_dim/hold.rs:118-179
  Rng rng{42, normal};
  const std::size_t n = 77;
  const std::vector<double> vals = rng.randn(n);
  const double start = -3.14, stop = 314.0;
  const std::vector<double> x_reg = linspace(start, stop, n);
  const auto g_reg = RegularGrid1D<double>::new_(x_reg[0], x_reg[1] - x_reg[0], vals).unwrap();
  auto left_reg = Left1D<RegularGrid1D<double>>::new_(g_reg).unwrap();
  auto right_reg = Right1D<RegularGrid1D<double>>::new_(g_reg).unwrap();
  auto nearest_reg = Nearest1D<RegularGrid1D<double>>::new_(g_reg).unwrap();
  std::vector<double> locs = rng.randn(3 * n);
  for (auto& x : locs) x = (x * 2.0 * (stop - start)) + 2.0 * start;
  const auto y_lreg = left_reg.eval_alloc(locs).unwrap();
  const auto y_rreg = right_reg.eval_alloc(locs).unwrap();
  const auto y_nreg = nearest_reg.eval_alloc(locs).unwrap();
  for (std::size_t i = 0; i < locs.size(); ++i) {
    const double loc = locs[i];
    const std::size_t j = cell_of(x_reg, loc);
    const double xleft = x_reg[j], xright = x_reg[j + 1], yleft = vals[j], yright = vals[j + 1];
    if (loc >= x_reg[0] && loc <= x_reg[n - 1]) {
      EXPECT(loc >= xleft && loc <= xright);
      EXPECT(y_lreg[i] == yleft);
      EXPECT(y_rreg[i] == yright);
    } else if (loc > x_reg[n - 1]) {
      EXPECT(y_lreg[i] == yright);
      EXPECT(y_rreg[i] == yright);
    } else if (loc < x_reg[0]) {
      EXPECT(y_lreg[i] == yleft);
      EXPECT(y_rreg[i] == yleft);
    }
    const double y_nearest = (loc - xleft) <= (xright - loc) ? yleft : yright;
    EXPECT(y_nreg[i] == y_nearest);
    EXPECT(left_reg.eval_one(loc).unwrap() == y_lreg[i]);
  }
}

static void linear_1d(bool normal) {  // one_dim/linear.rs:96-179
  Rng rng{7, normal};
  const std::size_t n = 77;
  const std::vector<double> vals = rng.randn(n);
  const double start = -3.14, stop = 314.0;
  const std::vector<double> x_reg = linspace(start, stop, n);
  const auto g_reg = RegularGrid1D<double>::new_(x_reg[0], x_reg[1] - x_reg[0], vals).unwrap();
  std::vector<double> x_rect = rng.randn(n);
  std::sort(x_rect.begin(), x_rect.end());
  for (auto& x : x_rect) x = (x * (stop - start)) + start;
  const auto g_rect = RectilinearGrid1D<double>::new_(x_rect, vals).unwrap();
  auto lin_reg = Linear1D<RegularGrid1D<double>>::new_(g_reg).unwrap();
  auto lin_rect = Linear1D<RectilinearGrid1D<double>>::new_(g_rect).unwrap();
  auto linhl_reg = LinearHoldLast1D<RegularGrid1D<double>>::new_(g_reg).unwrap();
  auto linhl_rect = LinearHoldLast1D<RectilinearGrid1D<double>>::new_(g_rect).unwrap();
  std::vector<double> locs = rng.randn(3 * n);
  for (auto& x : locs) x = (x * 2.0 * (stop - start)) + 2.0 * start;
  struct Case { const std::vector<double>* xs; std::vector<double> ys; bool hold; };
  const Case cases[] = {{&x_reg, lin_reg.eval_alloc(locs).unwrap(), false},
                        {&x_rect, lin_rect.eval_alloc(locs).unwrap(), false},
                        {&x_reg, linhl_reg.eval_alloc(locs).unwrap(), true},
                        {&x_rect, linhl_rect.eval_alloc(locs).unwrap(), true}};
  for (const Case& c : cases) {
    const std::vector<double>& xs = *c.xs;
    for (std::size_t i = 0; i < locs.size(); ++i) {
      const double loc = locs[i], y = c.ys[i];
      const std::size_t j = cell_of(xs, loc);
      const double xleft = xs[j], xright = xs[j + 1], yleft = vals[j], yright = vals[j + 1];
      const double slope = (yright - yleft) / (xright - xleft);
      const double dx = loc - xleft;
      const double ymax = std::max(yleft, yright), ymin = std::min(yleft, yright);
      if (loc >= xs[0] && loc <= xs[n - 1]) {
        EXPECT(y <= ymax && y >= ymin);
        EXPECT(loc >= xleft && loc <= xright);
      } else if (loc > xs[n - 1] && c.hold) {
        EXPECT(std::fabs((y - vals[n - 1]) / vals[n - 1]) < 1e-12);
        continue;
      } else if (loc < xs[0] && c.hold) {
        EXPECT(std::fabs((y - vals[0]) / vals[0]) < 1e-12);
        continue;
      }
      const double y_expected = yleft + slope * dx;
      EXPECT(std::fabs((y - y_expected) / y_expected) < 1e-12);
    }
  }
}

static void error_strings() {  // one_dim/mod.rs:53, :88, :111, :150
  const std::vector<double> vals{1.0, 2.0, 4.0}, grid{0.0, 1.0, 3.0}, short_grid{0.0, 1.0};
  auto bad = RectilinearGrid1D<double>::new_(short_grid, vals);
  EXPECT(bad.is_err() && std::strcmp(bad.err(), "Length mismatch") == 0);
  auto one = RectilinearGrid1D<double>::new_(Slice<double>(grid.data(), 1), Slice<double>(vals.data(), 1));
  EXPECT(one.is_err() && std::strcmp(one.err(), "Length mismatch") == 0);
  const auto g = RegularGrid1D<double>::new_(0.0, 1.0, vals).unwrap();
  auto lin = Linear1D<RegularGrid1D<double>>::new_(g).unwrap();
  std::vector<double> out(2, -1.0);
  auto r = lin.eval(grid, out);  // 3 locs, 2 outputs
  EXPECT(r.is_err() && std::strcmp(r.err(), "Length mismatch") == 0);
  const std::vector<double> locs{0.5, 1.5, NAN, 2.5};
  std::vector<double> out4(4, -1.0);
  auto u = lin.eval(locs, out4);
  EXPECT(u.is_err() && std::strcmp(u.err(), "Unrepresentable number") == 0);
  EXPECT(out4[0] == 1.5 && out4[1] == 3.0 && out4[2] == -1.0 && out4[3] == -1.0);  // stops at the first failing point
  EXPECT(lin.eval_one(INFINITY).is_err());
  EXPECT(std::strcmp(lin.eval_alloc(locs).err(), "Unrepresentable number") == 0);
  // a regular grid of one value: the reference panics at the first point (vals.len() - 2 underflows)
  const auto g1 = RegularGrid1D<double>::new_(0.0, 1.0, Slice<double>(vals.data(), 1)).unwrap();
  EXPECT(Left1D<RegularGrid1D<double>>::new_(g1).status() == INTERPN_HIP_ERR_REFERENCE_PANIC);
  // rectilinear grids never fail a point: NaN takes cell 0 (Left1D: vals[0]), +inf holds the last value
  const auto gr = RectilinearGrid1D<double>::new_(grid, vals).unwrap();
  auto left = Left1D<RectilinearGrid1D<double>>::new_(gr).unwrap();
  EXPECT(left.eval_one(NAN).unwrap() == 1.0 && left.eval_one(INFINITY).unwrap() == 4.0);
  // f32
  const std::vector<float> vf{1.0f, 2.0f, 4.0f};
  auto lf = Linear1D<RegularGrid1D<float>>::new_(RegularGrid1D<float>::new_(0.0f, 1.0f, vf).unwrap()).unwrap();
  EXPECT(lf.eval_one(2.5f).unwrap() == 5.0f);
}

int main() {
  if (interpn_hip_device_count() < 1) {
    std::printf("no HIP device: the library has no CPU path\n");
    return 2;
  }
  run("one_dim::hold test_hold_1d", [] { hold_1d(false); });
  run("one_dim::hold test_hold_1d (normal points)", [] { hold_1d(true); });
  run("one_dim::linear test_linear_1d", [] { linear_1d(false); });
  run("one_dim::linear test_linear_1d (normal points)", [] { linear_1d(true); });
  run("one_dim error strings", error_strings);
  if (g_failures == 0) std::printf("ALL PASSED\n");
  return g_failures == 0 ? 0 : 1;
}
