"""The one_dim part of the C++ mirror (include/interpn_hip.hpp: interpn_hip::one_dim and its re-exports) and the
reference's one_dim unit tests re-created against it (tests/cpp/one_dim_tests.cpp).

CPU tier: the header with the one_dim types and the test program compile in C++17 pedantic mode with warnings as
errors, with plain g++, and the program refuses to run without a device.  GPU tier: every re-created test passes."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "interpn_amd")
GXX = ["g++", "-std=c++17", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include")]
LINK = ["-L", LIBDIR, "-linterpn_hip", f"-Wl,-rpath,{LIBDIR}"]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def build(tmp_path, extra=()):
    exe = str(tmp_path / "one_dim_tests")
    subprocess.check_call([*GXX, "-O1", os.path.join(ROOT, "tests", "cpp", "one_dim_tests.cpp"), *LINK, "-o", exe, *extra])
    return exe


def test_one_dim_mirror_compiles_pedantic(tmp_path):
    """Every one_dim type, in both element types and through the root re-exports, in a pedantic translation unit."""
    probe = tmp_path / "probe.cpp"
    probe.write_text(r'''#include "interpn_hip.hpp"
#include <cstring>
int main() {
  using namespace interpn_hip;
  std::vector<double> v{1.0, 2.0, 4.0}, g{0.0, 1.0, 3.0};
  std::vector<float> vf{1.0f, 2.0f}, gf{0.0f};
  auto rg = one_dim::RegularGrid1D<double>::new_(0.0, 1.0, v).unwrap();
  auto cg = RectilinearGrid1D<double>::new_(g, v).unwrap();
  auto bad = one_dim::RectilinearGrid1D<float>::new_(gf, vf);
  one_dim::Extrap e = one_dim::Extrap::OutsideHigh;
  (void)e;
  auto a = one_dim::hold::Left1D<RegularGrid1D<double>>::new_(rg);
  auto b = one_dim::hold::Right1D<one_dim::RectilinearGrid1D<double>>::new_(cg);
  auto c = Nearest1D<RegularGrid1D<double>>::new_(rg, 0);
  auto d = one_dim::linear::Linear1D<RectilinearGrid1D<double>>::new_(cg);
  auto f = LinearHoldLast1D<RegularGrid1D<float>>::new_(RegularGrid1D<float>::new_(0.0f, 1.0f, vf).unwrap());
  if (d.is_ok()) {
    Result<std::vector<double>> r = d.unwrap().eval_alloc(g);
    Result<double> one = d.unwrap().eval_one(0.5);
    std::vector<double> out(3);
    Result<void> w = d.unwrap().eval(g, out);
    (void)r; (void)one; (void)w;
  }
  (void)a; (void)b; (void)c; (void)f;
  return bad.is_err() && std::strcmp(bad.err(), "Length mismatch") == 0 ? 0 : 1;
}
''')
    subprocess.check_call([*GXX, str(probe), *LINK, "-o", str(tmp_path / "probe")])
    assert subprocess.run([str(tmp_path / "probe")], timeout=120).returncode == 0
    assert os.path.exists(build(tmp_path))


def test_one_dim_tests_refuse_without_a_device(tmp_path):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    res = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and "no HIP device" in res.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("feature", [None, "1", "0"], ids=["default", "fma", "nofma"])
def test_reference_one_dim_tests_through_the_cpp_mirror(tmp_path, feature):
    """test_hold_1d (one_dim/hold.rs:118-179), test_linear_1d (one_dim/linear.rs:96-179) and the error strings, with the
    `fma` feature left to the process default or chosen at compile time."""
    extra = () if feature is None else (f"-DINTERPN_HIP_FEATURE_FMA={feature}",)
    res = subprocess.run([build(tmp_path, extra)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ALL PASSED" in res.stdout and "FAIL" not in res.stdout
    assert res.stdout.count("PASS ") == 5
