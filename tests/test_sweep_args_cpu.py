"""The host-side helpers that fill every sweep launcher's arguments (interpn_amd/csrc/sweep_rounds.h: sweep_key,
sweep_key_shift, step_reciprocals), compiled for the host and compared with the expressions the four launchers
used to write out by hand, on steps and spans from ordinary grids to the edges of StepCellRange and beyond.

One place may differ, and only there: step_reciprocals tests the step rounded to T (what the kernels divide by,
as the 3-D multilinear launcher did); the other launchers tested the double.  For f64 these are the same test;
for f32 they differ exactly where a double step rounds onto 2^16 or 2^-16.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "interpn_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "sweep_rounds.h"

using namespace interpn;

template <typename T> static bool same(T a, T b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }

// the launchers' own lines before the helpers
template <typename T> static void old_key(const GridDesc& g, int d, T* start, T* scale) {
  if (g.kind == kRectilinear) {
    const double span = g.bound_hi[d] - g.bound_lo[d];
    *start = (T)g.bound_lo[d];
    *scale = span > 0 ? (T)((double)(g.n[d] - 1) / span) : (T)0;
  } else {
    *start = (T)g.start[d];
    *scale = (T)(1.0 / g.step[d]);
  }
  if (!(*scale > 0) || !(*scale < (T)1e30)) *scale = 0;
}
template <typename T> static bool old_fast_rounded(double step) {  // k_linear_sweep.hip
  const T st = (T)step;
  const double mag = st < 0 ? -(double)st : (double)st;
  return mag >= StepCellRange<T>::lo && mag <= StepCellRange<T>::hi;
}
template <typename T> static bool old_fast_double(double step) {  // k_linear2_brick.hip, k_nearest.hip, k_cubic_sweep.hip
  const double mag = step < 0 ? -step : step;
  return mag >= StepCellRange<T>::lo && mag <= StepCellRange<T>::hi;
}

static long bad = 0, boundary = 0, cases = 0;

template <typename T> static void check(const std::vector<double>& steps) {
  for (size_t i = 0; i + 3 <= steps.size(); ++i) {
    GridDesc g;
    g.kind = kRegular;
    bool rounded = true, dbl = true;
    for (int d = 0; d < 3; ++d) {
      g.step[d] = steps[i + d];
      g.start[d] = -0.5 * (double)(i % 7);
      rounded = rounded && old_fast_rounded<T>(g.step[d]);
      dbl = dbl && old_fast_double<T>(g.step[d]);
    }
    T rstep[3];
    unsigned fastdiv = 7;
    step_reciprocals(g, rstep, &fastdiv);
    for (int d = 0; d < 3; ++d) {
      const volatile T one = (T)1;
      if (!same(rstep[d], (T)(one / (T)g.step[d]))) ++bad;
    }
    if (fastdiv != (rounded ? 1u : 0u)) ++bad;
    if (fastdiv != (dbl ? 1u : 0u)) {
      bool on_edge = false;
      for (int d = 0; d < 3; ++d) {
        const double r = std::fabs((double)(T)g.step[d]);
        on_edge = on_edge || r == StepCellRange<T>::lo || r == StepCellRange<T>::hi;
      }
      if (sizeof(T) == 8 || !on_edge) ++bad;
      ++boundary;
    }
    g.kind = kRectilinear;
    step_reciprocals(g, rstep, &fastdiv);
    for (int d = 0; d < 3; ++d)
      if (!same(rstep[d], (T)0)) ++bad;
    if (fastdiv != 0u) ++bad;
    for (int kind = 0; kind < 2; ++kind) {
      g.kind = kind;
      for (int d = 0; d < 3; ++d) {
        g.n[d] = 2 + (int)((i * 37 + (size_t)d * 101) % 5000);
        g.bound_lo[d] = g.start[d];
        g.bound_hi[d] = g.start[d] + steps[i + d] * (g.n[d] - 1);
        T s0, c0, s1, c1;
        old_key(g, d, &s0, &c0);
        sweep_key(g, d, &s1, &c1);
        if (!same(s0, s1) || !same(c0, c1)) ++bad;
        int shift = 0;
        while (((g.n[d] - 2) >> shift) >= 64) ++shift;
        if (sweep_key_shift(g.n[d] - 2) != shift) ++bad;
      }
      ++cases;
    }
  }
}

int main() {
  std::vector<double> steps = {1.0 / 63, 2.0 / 63, 0.1, 1.0, 3.0, -0.25, 0.0, -0.0, NAN, INFINITY, -INFINITY, 1e-300, 1e300,
                               0x1p-128, 0x1p128, 0x1p-16, 0x1p16, -0x1p16, -0x1p-16};
  for (double e : {0x1p-128, 0x1p128, 0x1p-16, 0x1p16})
    for (int k = -40; k <= 40; ++k) steps.push_back(std::nextafter(e, k < 0 ? 0.0 : INFINITY) * (1.0 + k * 0x1p-30));
  for (double e : {0x1p-16, 0x1p16})  // doubles that round onto the f32 edges from outside the range
    for (int k = 1; k <= 20; ++k) steps.push_back(e < 1 ? e * (1.0 - k * 0x1p-30) : e * (1.0 + k * 0x1p-30));
  std::mt19937_64 rng(7);
  std::uniform_real_distribution<double> m(1.0, 2.0);
  std::uniform_int_distribution<int> ex(-140, 140);
  for (int i = 0; i < 20000; ++i) steps.push_back(std::ldexp(m(rng), ex(rng)) * (i % 3 ? 1.0 : -1.0));
  check<double>(steps);
  check<float>(steps);
  std::printf("cases %ld boundary %ld bad %ld\n", cases, boundary, bad);
  return bad == 0 && cases > 0 ? 0 : 1;
}
"""


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_sweep_argument_helpers_match_the_launchers_former_expressions(tmp_path):
    src = tmp_path / "sweep_args.hip"
    src.write_text(PROGRAM)
    exe = tmp_path / "sweep_args"
    subprocess.check_call([HIPCC, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950",
                           "-I", CSRC, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    counts = dict(zip(out.stdout.split()[0::2], map(int, out.stdout.split()[1::2])))
    assert counts["bad"] == 0 and counts["cases"] > 40000
    assert counts["boundary"] > 0  # the f32 inputs that round onto the range's edges were exercised
