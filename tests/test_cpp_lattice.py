"""`interp_lattice` of the C++ mirror (include/interpn_hip.hpp) and its test program (tests/cpp/lattice_tests.cpp).

CPU tier: the header with the new member and the test program compile in C++17 pedantic mode with warnings as errors,
with plain g++, and the program refuses to run without a device.  GPU tier: every test of the program passes."""
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
    exe = str(tmp_path / "lattice_tests")
    subprocess.check_call([*GXX, "-O1", os.path.join(ROOT, "tests", "cpp", "lattice_tests.cpp"), *LINK, "-o", exe, *extra])
    return exe


def test_interp_lattice_compiles_pedantic(tmp_path):
    """The member on every mirror, both element types, in a pedantic translation unit; the C entry points from C++."""
    probe = tmp_path / "probe.cpp"
    probe.write_text(r'''#include "interpn_hip.hpp"
int main() {
  using namespace interpn_hip;
  MultilinearRegular<double, 3> a;
  MultilinearRectilinear<float, 2> b;
  MulticubicRegular<float, 3> c;
  MulticubicRectilinear<double, 2> d;
  NearestRegular<double, 4> e;
  NearestRectilinear<float, 1> f;
  std::vector<double> x{0.0, 1.0}, out(8);
  std::vector<float> xf{0.0f}, outf(1);
  // no handle behind the default-constructed mirrors: the C ABI says so
  int bad = 0;
  bad += a.interp_lattice({Slice<double>(x), Slice<double>(x), Slice<double>(x)}, out).status() != INTERPN_HIP_ERR_INVALID_ARGUMENT;
  bad += d.interp_lattice({Slice<double>(x), Slice<double>(x)}, out).status() != INTERPN_HIP_ERR_DIM_MISMATCH;  // 4 != 8
  bad += b.interp_lattice({Slice<float>(xf), Slice<float>(xf)}, outf).status() != INTERPN_HIP_ERR_INVALID_ARGUMENT;
  bad += c.interp_lattice({Slice<float>(xf), Slice<float>(xf), Slice<float>(xf)}, outf).is_ok();
  bad += f.interp_lattice({Slice<float>(xf)}, outf).is_ok();
  (void)e;
  std::size_t dims[2] = {64, 64}, lens[2] = {5000, 5000}, lds = 0, npts = 0;
  int path = -1;
  bad += interpn_hip_lattice_plan(8, INTERPN_HIP_LINEAR, 2, dims, lens, &path, &lds, &npts) != INTERPN_HIP_OK;
  bad += path != INTERPN_HIP_LATTICE_PATH_FUSED || lds != 4 * 64 * 8 || npts != 25000000;
  return bad;
}
''')
    subprocess.check_call([*GXX, str(probe), *LINK, "-o", str(tmp_path / "probe")])
    env = {k: v for k, v in os.environ.items() if not k.startswith("INTERPN_HIP_")}
    assert subprocess.run([str(tmp_path / "probe")], timeout=120, env=env).returncode == 0
    assert os.path.exists(build(tmp_path))


def test_lattice_tests_refuse_without_a_device(tmp_path):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    res = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and "no HIP device" in res.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("feature", [None, "1", "0"], ids=["default", "fma", "nofma"])
def test_lattice_tests_through_the_cpp_mirror(tmp_path, feature):
    """interp_lattice against interp on the expanded points for every mirror, with the `fma` feature left to the process
    default or chosen at compile time; the error contract."""
    extra = () if feature is None else (f"-DINTERPN_HIP_FEATURE_FMA={feature}",)
    res = subprocess.run([build(tmp_path, extra)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ALL PASSED" in res.stdout and "FAIL" not in res.stdout
    assert res.stdout.count("PASS ") == 6
