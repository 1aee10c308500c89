"""The k1 probe of tests/test_fma_sites_cpu.py on the GPU: tables on which 2 dy overflows in an end cell while 2 dy - k0 does
not (tests/helpers.py::k1_probe_case), so that `two.mul_add(dy, -k0)` and `two * dy - k0` — the same bits on every finite
workload of the suite — differ, and a kernel that takes the wrong form for a class returns inf or NaN where the reference is
finite, or the other way round.

Every result is compared bit for bit with the oracle (a NaN need only be a NaN; tests/family_runs.py::assert_same), and the
oracle's result is finite or not per class as the site table says (tests/golden/fma_sites.json): under `fma`, regular grids
fuse all four saturated classes in the flattened arm and all but OutsideLow in the recursive arm; rectilinear grids fuse none
in the flattened arm and InsideLow / InsideHigh in the recursive arm; without `fma` nothing is fused.  tests/test_fma_sites_cpu.py
holds the oracle itself against an exact-rational evaluation on the same inputs.

A case is 120 points (24 per saturated class of the probed axis and 24 in the cells between) on a grid of at most 4096 nodes;
every axis takes the role of the probed one in turn, with linearize_extrapolation off and on."""

import numpy as np
import pytest

from tests import cubic_grad_restatement as cg
from tests import family_runs as fr
from tests.family_runs import KNOBS
from tests.helpers import k1_assert_classes, k1_probe_case, run_hip_raw, run_oracle

pytestmark = pytest.mark.gpu

KINDS = ["regular", "rectilinear"]
N3, N5, N6 = [4, 5, 4], [4, 5, 4, 5, 4], [4, 4, 4, 4, 4, 4]
dtypes = pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
flavours = pytest.mark.parametrize("fma", [True, False], ids=["fma", "nofma"])
_WANT = {}  # the oracle on a probe case: computed once, shared by every form that runs the case


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for name in KNOBS:
        monkeypatch.delenv("INTERPN_HIP_" + name, raising=False)


def _probe(oracle, kind, shape, axis, dtype, fma, linearize):
    """(case, cls, want): the probe case, its points' classes, and the oracle's result — asserted to be finite exactly in
    the classes the site table gives for this grid kind, arm and flavour."""
    key = (kind, tuple(shape), axis, np.dtype(dtype).name, fma, linearize)
    case, cls = k1_probe_case(kind, shape, axis, dtype, linearize=linearize)
    if key not in _WANT:
        with np.errstate(all="ignore"):
            want = run_oracle(oracle, case, fma)
        k1_assert_classes(want, cls, kind, len(shape), fma, key)
        want.setflags(write=False)
        _WANT[key] = want
    return case, cls, _WANT[key]


def _cases(oracle, kind, shape, dtype, fma, linearizes=(False, True)):
    for axis in range(len(shape)):
        for linearize in linearizes:
            yield (axis, linearize), _probe(oracle, kind, shape, axis, dtype, fma, linearize)


# ---- the recursive arm: both forms of k_generic_n and the runtime-N kernel ------------------------------------------------------------------
@dtypes
@flavours
@pytest.mark.parametrize("form", ["onetree", "rowvec", "runtime"])
@pytest.mark.parametrize("shape", [N5, N6], ids=["N5", "N6"])
@pytest.mark.parametrize("kind", KINDS)
def test_recursive_arm(oracle, monkeypatch, kind, shape, form, fma, dtype):
    fr.recursive_arm_env(monkeypatch, form)
    n = len(shape)
    # the row-vector form exists where it fits the register file (k_generic.hip::generic_vec_ok); elsewhere the one-tree form runs
    rowvec = form == "rowvec" and (dtype == np.float32 or kind == "regular" or n == 5)
    for what, (case, cls, want) in _cases(oracle, kind, shape, dtype, fma):
        it = fr.make_handle(case, fma, monkeypatch)
        try:
            got = fr.eval_device(it, case.obs)
            name = it.kernel_name()
            assert it.last_path == "in_place"
            if form == "runtime":
                assert name.startswith("interpn::k_generic<"), name
            else:
                assert name.startswith("interpn::k_generic_n<") and name.endswith(", true>") == rowvec, name
            fr.assert_same(got, want, (name, what))
            fr.assert_same(it.eval_host(case.obs, np.zeros(want.size, dtype=dtype)), want, ("host", name, what))
        finally:
            it.close()
    if fma:  # the raw one-shot call (the `fma` flavour is its only one), once: on the last case
        fr.assert_same(run_hip_raw(case), want, ("raw", what))


# ---- value and gradient in one pass, N = 5 ----------------------------------------------------------------------------------------------------
@dtypes
@flavours
@pytest.mark.parametrize("linearize", [False, True], ids=["quad", "lin"])
@pytest.mark.parametrize("kind", KINDS)
def test_gradient_kernel_keeps_the_bits_of_eval(oracle, monkeypatch, kind, linearize, fma, dtype):
    import torch

    for what, (case, cls, want) in _cases(oracle, kind, N5, dtype, fma, (linearize,)):
        with np.errstate(all="ignore"):
            want_out, want_grad, ok = cg.eval_grad_case(case, fma=fma, dtype=dtype)
        assert ok.all()
        fr.assert_same(want_out, want, ("the restatement's value against the oracle", what))
        it = fr.make_handle(case, fma, monkeypatch)
        try:
            plain = fr.eval_device(it, case.obs)
            out, grad = it.eval_cubic_grad_tensors([torch.from_numpy(np.ascontiguousarray(o)).cuda() for o in case.obs])
            it.finish()
            name = it.kernel_name()
            assert name.startswith("interpn::k_cubic_grad_n<"), name
            out, grad = out.cpu().numpy(), grad.cpu().numpy()
            fr.assert_same(out, want, ("value", what))
            fr.assert_same(out, plain, ("value against eval", what))
            fr.assert_same(grad, want_grad, ("gradient", what))
        finally:
            it.close()


# ---- the flattened arm, N = 3: the C-order kernel, the tiled kernel, the sweep kernel, k_generic forced -----------------------------------
@dtypes
@flavours
@pytest.mark.parametrize("path", ["c_order", "tiles", "sweep", "generic"])
@pytest.mark.parametrize("kind", KINDS)
def test_flattened_arm(oracle, monkeypatch, kind, path, fma, dtype):
    if path == "generic":
        monkeypatch.setenv("INTERPN_HIP_FORCE_GENERIC", "1")
    for what, (case, cls, want) in _cases(oracle, kind, N3, dtype, fma):
        if path in ("c_order", "tiles"):
            fr.multicubic_c_order_and_tiles(case, want, fma, monkeypatch, kind, "off" if path == "c_order" else "11")
            continue
        it = fr.make_handle(case, fma, monkeypatch, "11" if path == "sweep" else None)
        try:
            if path == "sweep":
                it.set_option("sweep", 1)
            got = fr.eval_device(it, case.obs)
            name = it.kernel_name()
            if path == "sweep":
                assert it.last_path == "sweep", (it.last_path, it.last_path_reason)
                assert name.startswith("interpn::k_cubic_sweep<"), name
            else:
                assert name.startswith("interpn::k_generic<"), name
            fr.assert_same(got, want, (name, what))
        finally:
            it.close()
