"""What the Python front end raises for malformed calls, and with which words: a table of `(call, exception type, regex on
the message)` rows for the methods of `Interpolator` and `Fields` and for the module-level helpers.  Every row is decided
before the first call into the library or into CUDA, so objects with no handle behind them are enough; the tensor forms
are driven with a stand-in for a CUDA tensor that wraps a CPU tensor.  Where two checks could both fire, a row says which
one wins: the order of the checks is part of the behaviour."""

import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import interpn_amd  # noqa: E402
from interpn_amd import _lib  # noqa: E402

F64, F32 = torch.float64, torch.float32


class _Device:
    def __init__(self, index):
        self.index = index

    def __str__(self):
        return f"cuda:{self.index}"


class FakeCuda:
    """A CPU tensor that says it lives on cuda:`index`: enough for every check made in front of the library call."""

    is_cuda = True

    def __init__(self, t, index=0):
        self.t, self.device = t, _Device(index)

    dtype = property(lambda self: self.t.dtype)
    shape = property(lambda self: self.t.shape)

    def dim(self):
        return self.t.dim()

    def numel(self):
        return self.t.numel()

    def stride(self, *a):
        return self.t.stride(*a)

    def is_contiguous(self):
        return self.t.is_contiguous()

    def data_ptr(self):
        return self.t.data_ptr()

    def contiguous(self):
        return FakeCuda(self.t.contiguous(), self.device.index)

    def reshape(self, *a):
        return FakeCuda(self.t.reshape(*a), self.device.index)

    def __getitem__(self, i):
        return FakeCuda(self.t[i], self.device.index)


def cu(*shape, dtype=F64, dev=0):
    return FakeCuda(torch.zeros(shape, dtype=dtype), dev)


def ro(*shape):
    a = np.zeros(shape)
    a.flags.writeable = False
    return a


class It(interpn_amd.Interpolator):
    def device(self):
        return 0


class Fs(interpn_amd.Fields):
    def device(self):
        return 0

    def close(self):  # `fsl` below carries a made-up handle: there is nothing to destroy
        pass


class _OnlyStrerror:
    """Stands in for the loaded library: it knows the text of one status and nothing else, so a row that reaches any
    entry point fails with this AttributeError instead of the exception it lists."""

    @staticmethod
    def interpn_hip_strerror(status):
        assert status == _lib.ERR_DIM_MISMATCH, status
        return b"Dimension mismatch"

    def __getattr__(self, name):
        raise AttributeError(f"the row reached the library: {name}")


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: _OnlyStrerror())


it = It(0, np.float64, 3)       # N = 3
fs = Fs(0, np.float64, 2, 3)    # N = 2, K = 3
fsl = Fs(1, np.float64, 2, 3)   # the same: eval_lattice_tensors asks a set for its device only if its handle is not null

z = np.zeros
O3 = [z(5), z(5), z(5)]         # column-form points of `it`
O2 = [z(5), z(5)]               # ... of `fs`
A3 = [z(3), z(4), z(5)]         # lattice axes of `it`
A2 = [z(3), z(4)]               # ... of `fs`


def T3():
    return [cu(5), cu(5), cu(5)]


def T2():
    return [cu(5), cu(5)]


def TA3():
    return [cu(3), cu(4), cu(5)]


def TA2():
    return [cu(3), cu(4)]


CONTIG_1D = r"expected a contiguous 1-D torch\.float64 CUDA tensor"
PTS3 = r"pts: expected a 2-D torch\.float64 CUDA tensor of shape \(n, 3\) with stride\(1\) == 1 and stride\(0\) >= 3"
GRAD53 = r"grad: expected a 2-D torch\.float64 CUDA tensor of shape \(5, 3\) with stride\(1\) == 1 and stride\(0\) >= 3"
DIM = r"^Dimension mismatch$"
LIVES_IT = r" is on cuda:1 but this interpolator lives on cuda:0$"
LIVES_FS = r" is on cuda:1 but this set lives on cuda:0$"
F3264 = "`interpn` defined only for float32 and float64 data"

G = [np.linspace(0.0, 1.0, 4), np.linspace(0.0, 1.0, 5)]  # a 4 x 5 grid
V = z((4, 5))
VK = z((3, 4, 5))      # K = 3, fields first
VL = z((4, 5, 3))      # ... fields last
OB = [z(6), z(6)]
XI = z((6, 2))
AX = [z(3), z(6)]
PanicT = _lib.ReferencePanic

ROWS = [
    # ---- Interpolator.eval_host: `out` is looked at first, then the coordinate arrays ----
    ("it.eval_host/out-list", lambda: it.eval_host(O3, [0.0] * 5), TypeError, r"argument 'out': expected a numpy array, got list"),
    ("it.eval_host/out-dtype", lambda: it.eval_host(O3, z(5, np.float32)), TypeError, r"argument 'out': expected dtype float64, got float32"),
    ("it.eval_host/out-2d", lambda: it.eval_host(O3, z((5, 1))), TypeError, r"argument 'out': expected a 1-D array, got 2-D"),
    ("it.eval_host/out-strided", lambda: it.eval_host(O3, z(10)[::2]), ValueError, r"argument 'out': The given array is not contiguous"),
    ("it.eval_host/out-readonly", lambda: it.eval_host(O3, ro(5)), ValueError, r"argument 'out': array is read-only"),
    ("it.eval_host/obs-dtype", lambda: it.eval_host([z(5), z(5, np.float32), z(5)], z(5)), TypeError, r"argument 'obs\[1\]': expected dtype float64, got float32"),
    ("it.eval_host/obs-list", lambda: it.eval_host([z(5), z(5), [0.0] * 5], z(5)), TypeError, r"argument 'obs\[2\]': expected a numpy array, got list"),
    ("it.eval_host/obs-nine", lambda: it.eval_host([z(5)] * 9, z(5)), PanicT, r"argument 'obs': more than 8 arrays"),
    ("it.eval_host/out-before-obs", lambda: it.eval_host([[0.0] * 5] * 3, z(5, np.float32)), TypeError, r"argument 'out': expected dtype"),
    # ---- Interpolator.eval_tensors ----
    ("it.eval_tensors/obs-dtype", lambda: it.eval_tensors([cu(5), cu(5, dtype=F32), cu(5)], cu(5)), TypeError, r"^obs\[1\]: " + CONTIG_1D),
    ("it.eval_tensors/obs-strided", lambda: it.eval_tensors([cu(10)[::2], cu(5), cu(5)], cu(5)), TypeError, r"^obs\[0\]: " + CONTIG_1D),
    ("it.eval_tensors/obs-2d", lambda: it.eval_tensors([cu(5), cu(5), cu(5, 1)], cu(5)), TypeError, r"^obs\[2\]: " + CONTIG_1D),
    ("it.eval_tensors/obs-cpu", lambda: it.eval_tensors([torch.zeros(5, dtype=F64)] * 3, cu(5)), TypeError, r"^obs\[0\]: " + CONTIG_1D),
    ("it.eval_tensors/obs-device", lambda: it.eval_tensors([cu(5), cu(5, dev=1), cu(5)], cu(5)), ValueError, r"^obs\[1\]" + LIVES_IT),
    ("it.eval_tensors/device-of-0-before-dtype-of-1", lambda: it.eval_tensors([cu(5, dev=1), cu(5, dtype=F32), cu(5)], cu(5)), ValueError, r"^obs\[0\]" + LIVES_IT),
    ("it.eval_tensors/dtype-of-0-before-device-of-1", lambda: it.eval_tensors([cu(5, dtype=F32), cu(5, dev=1), cu(5)], cu(5)), TypeError, r"^obs\[0\]: " + CONTIG_1D),
    ("it.eval_tensors/obs-lengths", lambda: it.eval_tensors([cu(5), cu(4), cu(5)], cu(5)), AssertionError, DIM),
    ("it.eval_tensors/lengths-before-out", lambda: it.eval_tensors([cu(5), cu(4), cu(5)], cu(5, dtype=F32)), AssertionError, DIM),
    ("it.eval_tensors/out-dtype", lambda: it.eval_tensors(T3(), cu(5, dtype=F32)), TypeError, r"^out: " + CONTIG_1D),
    ("it.eval_tensors/out-strided", lambda: it.eval_tensors(T3(), cu(10)[::2]), TypeError, r"^out: " + CONTIG_1D),
    ("it.eval_tensors/out-length", lambda: it.eval_tensors(T3(), cu(4)), AssertionError, DIM),
    ("it.eval_tensors/out-device", lambda: it.eval_tensors(T3(), cu(5, dev=1)), ValueError, r"^out" + LIVES_IT),
    ("it.eval_tensors/out-length-before-device", lambda: it.eval_tensors(T3(), cu(4, dev=1)), AssertionError, DIM),
    # ---- Interpolator.eval_grad_host (and the cubic alias): the coordinate arrays first, then `out`, then `grad` ----
    ("it.eval_grad_host/obs-list", lambda: it.eval_grad_host([[0.0] * 5, z(5), z(5)], z(5), z((3, 5))), TypeError, r"argument 'obs\[0\]': expected a numpy array, got list"),
    ("it.eval_grad_host/obs-before-out", lambda: it.eval_grad_host([[0.0] * 5, z(5), z(5)], z(5, np.float32), z((3, 5))), TypeError, r"argument 'obs\[0\]'"),
    ("it.eval_grad_host/out-dtype", lambda: it.eval_grad_host(O3, z(5, np.float32), z((3, 5))), TypeError, r"argument 'out': expected dtype float64, got float32"),
    ("it.eval_grad_host/out-before-grad", lambda: it.eval_grad_host(O3, z(10)[::2], [0.0]), ValueError, r"argument 'out': The given array is not contiguous"),
    ("it.eval_grad_host/grad-list", lambda: it.eval_grad_host(O3, z(5), [[0.0] * 5] * 3), TypeError, r"argument 'grad': expected a numpy array, got list"),
    ("it.eval_grad_host/grad-dtype", lambda: it.eval_grad_host(O3, z(5), z((3, 5), np.float32)), TypeError, r"argument 'grad': expected dtype float64, got float32"),
    ("it.eval_grad_host/grad-dtype-before-shape", lambda: it.eval_grad_host(O3, z(5), z((3, 4), np.float32)), TypeError, r"argument 'grad': expected dtype"),
    ("it.eval_grad_host/grad-shape", lambda: it.eval_grad_host(O3, z(5), z((3, 4))), ValueError, r"^grad: expected shape \(3, 5\), got \(3, 4\)$"),
    ("it.eval_grad_host/grad-shape-by-out", lambda: it.eval_grad_host(O3, z(4), z((3, 5))), ValueError, r"^grad: expected shape \(3, 4\), got \(3, 5\)$"),
    ("it.eval_grad_host/grad-rows", lambda: it.eval_grad_host(O3, z(5), z((3, 10))[:, ::2]), ValueError, r"argument 'grad': every row must be contiguous"),
    ("it.eval_grad_host/grad-readonly", lambda: it.eval_grad_host(O3, z(5), ro(3, 5)), ValueError, r"argument 'grad': array is read-only"),
    ("it.eval_grad_host/rows-before-readonly", lambda: it.eval_grad_host(O3, z(5), ro(3, 10)[:, ::2]), ValueError, r"every row must be contiguous"),
    ("it.eval_cubic_grad_host/grad-shape", lambda: it.eval_cubic_grad_host(O3, z(5), z((5, 3))), ValueError, r"^grad: expected shape \(3, 5\), got \(5, 3\)$"),
    ("it.eval_cubic_grad_host/obs-dtype", lambda: it.eval_cubic_grad_host([z(5, np.float32)] * 3, z(5), z((3, 5))), TypeError, r"argument 'obs\[0\]': expected dtype"),
    # ---- Interpolator.eval_grad_tensors (and the cubic alias) ----
    ("it.eval_grad_tensors/obs-numpy", lambda: it.eval_grad_tensors(O3, cu(5), cu(3, 5)), TypeError, r"^obs\[0\]: " + CONTIG_1D),
    ("it.eval_grad_tensors/obs-device", lambda: it.eval_grad_tensors([cu(5), cu(5), cu(5, dev=1)], cu(5), cu(3, 5)), ValueError, r"^obs\[2\]" + LIVES_IT),
    ("it.eval_grad_tensors/obs-lengths", lambda: it.eval_grad_tensors([cu(5), cu(5), cu(6)], cu(5), cu(3, 5)), AssertionError, DIM),
    ("it.eval_grad_tensors/out-dtype", lambda: it.eval_grad_tensors(T3(), cu(5, dtype=F32), cu(3, 5)), TypeError, r"^out: " + CONTIG_1D),
    ("it.eval_grad_tensors/out-length", lambda: it.eval_grad_tensors(T3(), cu(6), cu(3, 5)), AssertionError, DIM),
    ("it.eval_grad_tensors/out-device", lambda: it.eval_grad_tensors(T3(), cu(5, dev=1), cu(3, 5)), ValueError, r"^out" + LIVES_IT),
    ("it.eval_grad_tensors/out-before-grad", lambda: it.eval_grad_tensors(T3(), cu(6), cu(3, 4)), AssertionError, DIM),
    ("it.eval_grad_tensors/grad-dtype", lambda: it.eval_grad_tensors(T3(), cu(5), cu(3, 5, dtype=F32)), TypeError, r"^grad: expected a 2-D torch\.float64 CUDA tensor with contiguous rows$"),
    ("it.eval_grad_tensors/grad-1d", lambda: it.eval_grad_tensors(T3(), cu(5), cu(15)), TypeError, r"^grad: expected a 2-D torch\.float64 CUDA tensor with contiguous rows$"),
    ("it.eval_grad_tensors/grad-rows", lambda: it.eval_grad_tensors(T3(), cu(5), cu(3, 10)[:, ::2]), TypeError, r"^grad: expected a 2-D torch\.float64 CUDA tensor with contiguous rows$"),
    ("it.eval_grad_tensors/grad-shape", lambda: it.eval_grad_tensors(T3(), cu(5), cu(3, 4)), ValueError, r"^grad: expected shape \(3, 5\), got \(3, 4\)$"),
    ("it.eval_grad_tensors/grad-rows-before-shape", lambda: it.eval_grad_tensors(T3(), cu(5), cu(3, 8)[:, ::2]), TypeError, r"with contiguous rows$"),
    ("it.eval_grad_tensors/grad-device", lambda: it.eval_grad_tensors(T3(), cu(5), cu(3, 5, dev=1)), ValueError, r"^grad" + LIVES_IT),
    ("it.eval_grad_tensors/grad-shape-before-device", lambda: it.eval_grad_tensors(T3(), cu(5), cu(3, 4, dev=1)), ValueError, r"^grad: expected shape"),
    ("it.eval_cubic_grad_tensors/grad-shape", lambda: it.eval_cubic_grad_tensors(T3(), cu(5), cu(5, 3)), ValueError, r"^grad: expected shape \(3, 5\), got \(5, 3\)$"),
    ("it.eval_cubic_grad_tensors/obs-numpy", lambda: it.eval_cubic_grad_tensors(O3, cu(5), cu(3, 5)), TypeError, r"^obs\[0\]: " + CONTIG_1D),
    # ---- Interpolator.eval_points_host: the width is looked at before the strides ----
    ("it.eval_points_host/pts-list", lambda: it.eval_points_host([[0.0] * 3], z(1)), TypeError, r"argument 'pts': expected a numpy array, got list"),
    ("it.eval_points_host/pts-dtype", lambda: it.eval_points_host(z((5, 3), np.float32), z(5)), TypeError, r"argument 'pts': expected dtype float64, got float32"),
    ("it.eval_points_host/pts-1d", lambda: it.eval_points_host(z(15), z(5)), TypeError, r"argument 'pts': expected a 2-D array of shape \(n, 3\), got 1 dimension\(s\)"),
    ("it.eval_points_host/pts-width", lambda: it.eval_points_host(z((5, 4)), z(5)), AssertionError, DIM),
    ("it.eval_points_host/width-before-rows", lambda: it.eval_points_host(z((5, 8))[:, ::2], z(5)), AssertionError, DIM),
    ("it.eval_points_host/pts-rows", lambda: it.eval_points_host(z((5, 6))[:, ::2], z(5)), ValueError, r"argument 'pts': every row must be contiguous"),
    ("it.eval_points_host/pts-rows-of-an-empty-array", lambda: it.eval_points_host(z((0, 6))[:, ::2], z(0)), ValueError, r"argument 'pts': every row must be contiguous"),
    ("it.eval_points_host/pts-row-stride", lambda: it.eval_points_host(z((5, 3))[::-1], z(5)), ValueError, r"argument 'pts': the row stride must be a whole number of elements, at least 3"),
    ("it.eval_points_host/pts-row-stride-0", lambda: it.eval_points_host(np.broadcast_to(z(3), (5, 3)), z(5)), ValueError, r"argument 'pts': the row stride must be a whole number of elements, at least 3"),
    ("it.eval_points_host/pts-before-out", lambda: it.eval_points_host(z((5, 6))[:, ::2], z(4)), ValueError, r"argument 'pts': every row"),
    ("it.eval_points_host/out-dtype", lambda: it.eval_points_host(z((5, 3)), z(5, np.float32)), TypeError, r"argument 'out': expected dtype float64, got float32"),
    ("it.eval_points_host/out-length", lambda: it.eval_points_host(z((5, 3)), z(4)), AssertionError, DIM),
    ("it.eval_points_host/out-readonly-before-length", lambda: it.eval_points_host(z((5, 3)), ro(4)), ValueError, r"argument 'out': array is read-only"),
    # ---- Interpolator.eval_points_tensors: the strides are looked at before the width ----
    ("it.eval_points_tensors/pts-numpy", lambda: it.eval_points_tensors(z((5, 3)), cu(5)), TypeError, "^" + PTS3 + "$"),
    ("it.eval_points_tensors/pts-1d", lambda: it.eval_points_tensors(cu(15), cu(5)), TypeError, "^" + PTS3 + "$"),
    ("it.eval_points_tensors/pts-dtype", lambda: it.eval_points_tensors(cu(5, 3, dtype=F32), cu(5)), TypeError, "^" + PTS3 + "$"),
    ("it.eval_points_tensors/pts-rows", lambda: it.eval_points_tensors(cu(5, 6)[:, ::2], cu(5)), TypeError, "^" + PTS3 + "$"),
    ("it.eval_points_tensors/pts-row-stride", lambda: it.eval_points_tensors(FakeCuda(torch.zeros(3, dtype=F64).expand(5, 3)), cu(5)), TypeError, "^" + PTS3 + "$"),
    ("it.eval_points_tensors/pts-width", lambda: it.eval_points_tensors(cu(5, 4), cu(5)), AssertionError, DIM),
    ("it.eval_points_tensors/rows-before-width", lambda: it.eval_points_tensors(cu(5, 8)[:, ::2], cu(5)), TypeError, "^" + PTS3 + "$"),
    ("it.eval_points_tensors/pts-device", lambda: it.eval_points_tensors(cu(5, 3, dev=1), cu(5)), ValueError, r"^pts" + LIVES_IT),
    ("it.eval_points_tensors/width-before-device", lambda: it.eval_points_tensors(cu(5, 4, dev=1), cu(5)), AssertionError, DIM),
    ("it.eval_points_tensors/out-dtype", lambda: it.eval_points_tensors(cu(5, 3), cu(5, dtype=F32)), TypeError, r"^out: " + CONTIG_1D),
    ("it.eval_points_tensors/out-length", lambda: it.eval_points_tensors(cu(5, 3), cu(4)), AssertionError, DIM),
    ("it.eval_points_tensors/out-device", lambda: it.eval_points_tensors(cu(5, 3), cu(5, dev=1)), ValueError, r"^out" + LIVES_IT),
    # ---- Interpolator.eval_points_grad_host ----
    ("it.eval_points_grad_host/pts-list", lambda: it.eval_points_grad_host([[0.0] * 3], z(1), z((1, 3))), TypeError, r"argument 'pts': expected a numpy array, got list"),
    ("it.eval_points_grad_host/pts-dtype", lambda: it.eval_points_grad_host(z((5, 3), np.float32), z(5), z((5, 3))), TypeError, r"argument 'pts': expected dtype float64, got float32"),
    ("it.eval_points_grad_host/pts-3d", lambda: it.eval_points_grad_host(z((5, 1, 3)), z(5), z((5, 3))), TypeError, r"argument 'pts': expected a 2-D array of shape \(n, 3\), got 3 dimension\(s\)"),
    ("it.eval_points_grad_host/pts-width", lambda: it.eval_points_grad_host(z((5, 2)), z(5), z((5, 3))), AssertionError, DIM),
    ("it.eval_points_grad_host/pts-rows", lambda: it.eval_points_grad_host(z((5, 6))[:, ::2], z(5), z((5, 3))), ValueError, r"argument 'pts': every row must be contiguous"),
    ("it.eval_points_grad_host/pts-row-stride", lambda: it.eval_points_grad_host(z((5, 3))[::-1], z(5), z((5, 3))), ValueError, r"argument 'pts': the row stride must be a whole number of elements, at least 3"),
    ("it.eval_points_grad_host/out-length", lambda: it.eval_points_grad_host(z((5, 3)), z(6), z((5, 3))), AssertionError, DIM),
    ("it.eval_points_grad_host/out-before-grad", lambda: it.eval_points_grad_host(z((5, 3)), z(6), [0.0]), AssertionError, DIM),
    ("it.eval_points_grad_host/grad-list", lambda: it.eval_points_grad_host(z((5, 3)), z(5), [[0.0] * 3] * 5), TypeError, r"argument 'grad': expected a numpy array, got list"),
    ("it.eval_points_grad_host/grad-dtype", lambda: it.eval_points_grad_host(z((5, 3)), z(5), z((5, 3), np.float32)), TypeError, r"argument 'grad': expected dtype float64, got float32"),
    ("it.eval_points_grad_host/grad-shape", lambda: it.eval_points_grad_host(z((5, 3)), z(5), z((5, 4))), ValueError, r"^grad: expected shape \(5, 3\), got \(5, 4\)$"),
    ("it.eval_points_grad_host/grad-readonly", lambda: it.eval_points_grad_host(z((5, 3)), z(5), ro(5, 3)), ValueError, r"argument 'grad': array is read-only"),
    ("it.eval_points_grad_host/grad-rows", lambda: it.eval_points_grad_host(z((5, 3)), z(5), z((5, 6))[:, ::2]), ValueError, r"argument 'grad': every row must be contiguous"),
    ("it.eval_points_grad_host/grad-row-stride", lambda: it.eval_points_grad_host(z((5, 3)), z(5), z((5, 3))[::-1]), ValueError, r"argument 'grad': the row stride must be a whole number of elements, at least 3"),
    ("it.eval_points_grad_host/readonly-before-rows", lambda: it.eval_points_grad_host(z((5, 3)), z(5), ro(5, 6)[:, ::2]), ValueError, r"argument 'grad': array is read-only"),
    # ---- Interpolator.eval_points_grad_tensors ----
    ("it.eval_points_grad_tensors/pts-numpy", lambda: it.eval_points_grad_tensors(z((5, 3)), cu(5), cu(5, 3)), TypeError, "^" + PTS3 + "$"),
    ("it.eval_points_grad_tensors/pts-rows", lambda: it.eval_points_grad_tensors(cu(5, 6)[:, ::2], cu(5), cu(5, 3)), TypeError, "^" + PTS3 + "$"),
    ("it.eval_points_grad_tensors/pts-width", lambda: it.eval_points_grad_tensors(cu(5, 2), cu(5), cu(5, 3)), AssertionError, DIM),
    ("it.eval_points_grad_tensors/pts-device", lambda: it.eval_points_grad_tensors(cu(5, 3, dev=1), cu(5), cu(5, 3)), ValueError, r"^pts" + LIVES_IT),
    ("it.eval_points_grad_tensors/out-dtype", lambda: it.eval_points_grad_tensors(cu(5, 3), cu(5, dtype=F32), cu(5, 3)), TypeError, r"^out: " + CONTIG_1D),
    ("it.eval_points_grad_tensors/out-length", lambda: it.eval_points_grad_tensors(cu(5, 3), cu(6), cu(5, 3)), AssertionError, DIM),
    ("it.eval_points_grad_tensors/out-device", lambda: it.eval_points_grad_tensors(cu(5, 3), cu(5, dev=1), cu(5, 3)), ValueError, r"^out" + LIVES_IT),
    ("it.eval_points_grad_tensors/grad-numpy", lambda: it.eval_points_grad_tensors(cu(5, 3), cu(5), z((5, 3))), TypeError, "^" + GRAD53 + "$"),
    ("it.eval_points_grad_tensors/grad-dtype", lambda: it.eval_points_grad_tensors(cu(5, 3), cu(5), cu(5, 3, dtype=F32)), TypeError, "^" + GRAD53 + "$"),
    ("it.eval_points_grad_tensors/grad-width", lambda: it.eval_points_grad_tensors(cu(5, 3), cu(5), cu(5, 4)), ValueError, r"^grad: expected shape \(5, 3\), got \(5, 4\)$"),
    ("it.eval_points_grad_tensors/grad-rows", lambda: it.eval_points_grad_tensors(cu(5, 3), cu(5), cu(5, 6)[:, ::2]), TypeError, "^" + GRAD53 + "$"),
    ("it.eval_points_grad_tensors/grad-row-stride", lambda: it.eval_points_grad_tensors(cu(5, 3), cu(5), FakeCuda(torch.zeros(3, dtype=F64).expand(5, 3))), TypeError, "^" + GRAD53 + "$"),
    ("it.eval_points_grad_tensors/shape-before-rows", lambda: it.eval_points_grad_tensors(cu(5, 3), cu(5), cu(5, 8)[:, ::2]), ValueError, r"^grad: expected shape \(5, 3\), got \(5, 4\)$"),
    ("it.eval_points_grad_tensors/grad-device", lambda: it.eval_points_grad_tensors(cu(5, 3), cu(5), cu(5, 3, dev=1)), ValueError, r"^grad" + LIVES_IT),
    ("it.eval_points_grad_tensors/rows-before-device", lambda: it.eval_points_grad_tensors(cu(5, 3), cu(5), cu(5, 6, dev=1)[:, ::2]), TypeError, "^" + GRAD53 + "$"),
    # ---- Interpolator.eval_lattice_host ----
    ("it.eval_lattice_host/axes-dtype", lambda: it.eval_lattice_host([z(3), z(4, np.float32), z(5)], z((3, 4, 5))), TypeError, r"argument 'axes\[1\]': expected dtype float64, got float32"),
    ("it.eval_lattice_host/axes-before-out", lambda: it.eval_lattice_host([z(3), z(4), z((5, 1))], [0.0]), TypeError, r"argument 'axes\[2\]': expected a 1-D array, got 2-D"),
    ("it.eval_lattice_host/out-list", lambda: it.eval_lattice_host(A3, [0.0] * 60), TypeError, r"argument 'out': expected a numpy array, got list"),
    ("it.eval_lattice_host/out-dtype", lambda: it.eval_lattice_host(A3, z((3, 4, 5), np.float32)), TypeError, r"argument 'out': expected dtype float64, got float32"),
    ("it.eval_lattice_host/out-shape", lambda: it.eval_lattice_host(A3, z((3, 5, 4))), ValueError, r"^out: expected shape \(3, 4, 5\), got \(3, 5, 4\)$"),
    ("it.eval_lattice_host/dtype-before-shape", lambda: it.eval_lattice_host(A3, z((3, 5, 4), np.float32)), TypeError, r"argument 'out': expected dtype"),
    ("it.eval_lattice_host/out-strided", lambda: it.eval_lattice_host(A3, z((3, 4, 10))[:, :, ::2]), ValueError, r"argument 'out': The given array is not contiguous"),
    ("it.eval_lattice_host/out-readonly", lambda: it.eval_lattice_host(A3, ro(3, 4, 5)), ValueError, r"argument 'out': array is read-only"),
    ("it.eval_lattice_host/strided-before-readonly", lambda: it.eval_lattice_host(A3, ro(3, 4, 10)[:, :, ::2]), ValueError, r"not contiguous"),
    # ---- Interpolator.eval_lattice_tensors: the axes need not be equally long ----
    ("it.eval_lattice_tensors/axes-numpy", lambda: it.eval_lattice_tensors(A3, cu(3, 4, 5)), TypeError, r"^axes\[0\]: " + CONTIG_1D),
    ("it.eval_lattice_tensors/axes-dtype", lambda: it.eval_lattice_tensors([cu(3), cu(4, dtype=F32), cu(5)], cu(3, 4, 5)), TypeError, r"^axes\[1\]: " + CONTIG_1D),
    ("it.eval_lattice_tensors/axes-device", lambda: it.eval_lattice_tensors([cu(3), cu(4), cu(5, dev=1)], cu(3, 4, 5)), ValueError, r"^axes\[2\]" + LIVES_IT),
    ("it.eval_lattice_tensors/out-dtype", lambda: it.eval_lattice_tensors(TA3(), cu(3, 4, 5, dtype=F32)), TypeError, r"^out: expected a contiguous torch\.float64 CUDA tensor$"),
    ("it.eval_lattice_tensors/out-strided", lambda: it.eval_lattice_tensors(TA3(), cu(3, 4, 10)[:, :, ::2]), TypeError, r"^out: expected a contiguous torch\.float64 CUDA tensor$"),
    ("it.eval_lattice_tensors/out-shape", lambda: it.eval_lattice_tensors(TA3(), cu(3, 5, 4)), ValueError, r"^out: expected shape \(3, 4, 5\), got \(3, 5, 4\)$"),
    ("it.eval_lattice_tensors/out-device", lambda: it.eval_lattice_tensors(TA3(), cu(3, 4, 5, dev=1)), ValueError, r"^out" + LIVES_IT),
    ("it.eval_lattice_tensors/shape-before-device", lambda: it.eval_lattice_tensors(TA3(), cu(3, 5, 4, dev=1)), ValueError, r"^out: expected shape"),
    # ---- Interpolator.check_bounds_tensors ----
    ("it.check_bounds_tensors/obs-dtype", lambda: it.check_bounds_tensors([cu(5), cu(5, dtype=F32), cu(5)], 1e-8), TypeError, r"^obs\[1\]: " + CONTIG_1D),
    ("it.check_bounds_tensors/obs-device", lambda: it.check_bounds_tensors([cu(5, dev=1), cu(5), cu(5)], 1e-8), ValueError, r"^obs\[0\]" + LIVES_IT),
    ("it.check_bounds_tensors/obs-lengths", lambda: it.check_bounds_tensors([cu(5), cu(5), cu(4)], 1e-8), AssertionError, DIM),

    # ---- Fields.eval_host ----
    ("fs.eval_host/obs-list", lambda: fs.eval_host([[0.0] * 5, z(5)], z((3, 5))), TypeError, r"argument 'obs\[0\]': expected a numpy array, got list"),
    ("fs.eval_host/obs-before-out", lambda: fs.eval_host([z(5), z(5, np.float32)], z((5, 3))), TypeError, r"argument 'obs\[1\]': expected dtype"),
    ("fs.eval_host/out-shape", lambda: fs.eval_host(O2, z((5, 3))), ValueError, r"^out: expected a \(3, 5\) array of float64$"),
    ("fs.eval_host/out-dtype", lambda: fs.eval_host(O2, z((3, 5), np.float32)), ValueError, r"^out: expected a \(3, 5\) array of float64$"),
    ("fs.eval_host/out-list", lambda: fs.eval_host(O2, [[0.0] * 5] * 3), ValueError, r"^out: expected a \(3, 5\) array of float64$"),
    ("fs.eval_host/out-rows", lambda: fs.eval_host(O2, z((3, 10))[:, ::2]), ValueError, r"^out: rows must be contiguous$"),
    ("fs.eval_host/out-row-stride", lambda: fs.eval_host(O2, z((3, 5))[::-1]), ValueError, r"^out: rows must be contiguous$"),
    ("fs.eval_host/out-readonly", lambda: fs.eval_host(O2, ro(3, 5)), ValueError, r"^out: array is read-only$"),
    ("fs.eval_host/rows-before-readonly", lambda: fs.eval_host(O2, ro(3, 10)[:, ::2]), ValueError, r"^out: rows must be contiguous$"),
    # ---- Fields.eval_tensors: `out` is not asked for its device ----
    ("fs.eval_tensors/obs-dtype", lambda: fs.eval_tensors([cu(5), cu(5, dtype=F32)], cu(3, 5)), TypeError, r"^obs\[1\]: " + CONTIG_1D),
    ("fs.eval_tensors/obs-cpu", lambda: fs.eval_tensors([torch.zeros(5, dtype=F64)] * 2, cu(3, 5)), TypeError, r"^obs\[0\]: " + CONTIG_1D),
    ("fs.eval_tensors/obs-device", lambda: fs.eval_tensors([cu(5, dev=1), cu(5)], cu(3, 5)), ValueError, r"^obs\[0\]" + LIVES_FS),
    ("fs.eval_tensors/obs-lengths", lambda: fs.eval_tensors([cu(5), cu(6)], cu(3, 5)), AssertionError, DIM),
    ("fs.eval_tensors/out-dtype", lambda: fs.eval_tensors(T2(), cu(3, 5, dtype=F32)), TypeError, r"^out: expected a \(3, 5\) torch\.float64 CUDA tensor$"),
    ("fs.eval_tensors/out-shape", lambda: fs.eval_tensors(T2(), cu(5, 3)), TypeError, r"^out: expected a \(3, 5\) torch\.float64 CUDA tensor$"),
    ("fs.eval_tensors/out-rows", lambda: fs.eval_tensors(T2(), cu(3, 10)[:, ::2]), ValueError, r"^out: rows must be contiguous$"),
    ("fs.eval_tensors/out-row-stride", lambda: fs.eval_tensors(T2(), FakeCuda(torch.zeros(5, dtype=F64).expand(3, 5))), ValueError, r"^out: rows must be contiguous$"),
    # ---- Fields.eval_grad_host: both shapes, then the layouts, then read-only ----
    ("fs.eval_grad_host/obs-dtype", lambda: fs.eval_grad_host([z(5, np.float32), z(5)], z((3, 5)), z((3, 2, 5))), TypeError, r"argument 'obs\[0\]': expected dtype"),
    ("fs.eval_grad_host/out-shape", lambda: fs.eval_grad_host(O2, z((5, 3)), z((3, 2, 5))), ValueError, r"^out: expected a \(3, 5\) array of float64$"),
    ("fs.eval_grad_host/out-before-grad", lambda: fs.eval_grad_host(O2, z((5, 3)), z((3, 2, 6))), ValueError, r"^out: expected a \(3, 5\) array of float64$"),
    ("fs.eval_grad_host/grad-shape", lambda: fs.eval_grad_host(O2, z((3, 5)), z((3, 2, 6))), ValueError, r"^grad: expected a \(3, 2, 5\) array of float64$"),
    ("fs.eval_grad_host/grad-dtype", lambda: fs.eval_grad_host(O2, z((3, 5)), z((3, 2, 5), np.float32)), ValueError, r"^grad: expected a \(3, 2, 5\) array of float64$"),
    ("fs.eval_grad_host/grad-shape-before-out-rows", lambda: fs.eval_grad_host(O2, z((3, 10))[:, ::2], z((3, 2, 6))), ValueError, r"^grad: expected a \(3, 2, 5\)"),
    ("fs.eval_grad_host/out-rows", lambda: fs.eval_grad_host(O2, z((3, 10))[:, ::2], z((3, 2, 5))), ValueError, r"^out: rows must be contiguous$"),
    ("fs.eval_grad_host/grad-last-axis", lambda: fs.eval_grad_host(O2, z((3, 5)), z((3, 2, 10))[..., ::2]), ValueError, r"^grad: the last axis must be contiguous \(unit stride\)$"),
    ("fs.eval_grad_host/grad-uniform", lambda: fs.eval_grad_host(O2, z((3, 5)), z((3, 3, 5))[:, :2]), ValueError, r"^grad: one uniform stride of at least 5 elements between the K \* N rows"),
    ("fs.eval_grad_host/grad-readonly", lambda: fs.eval_grad_host(O2, z((3, 5)), ro(3, 2, 5)), ValueError, r"^out, grad: array is read-only$"),
    ("fs.eval_grad_host/out-readonly", lambda: fs.eval_grad_host(O2, ro(3, 5), z((3, 2, 5))), ValueError, r"^out, grad: array is read-only$"),
    ("fs.eval_grad_host/layout-before-readonly", lambda: fs.eval_grad_host(O2, z((3, 5)), ro(3, 2, 10)[..., ::2]), ValueError, r"^grad: the last axis"),
    # ---- Fields.eval_grad_tensors ----
    ("fs.eval_grad_tensors/obs-dtype", lambda: fs.eval_grad_tensors([cu(5, dtype=F32), cu(5)], cu(3, 5), cu(3, 2, 5)), TypeError, r"^obs\[0\]: " + CONTIG_1D),
    ("fs.eval_grad_tensors/obs-device", lambda: fs.eval_grad_tensors([cu(5), cu(5, dev=1)], cu(3, 5), cu(3, 2, 5)), ValueError, r"^obs\[1\]" + LIVES_FS),
    ("fs.eval_grad_tensors/obs-lengths", lambda: fs.eval_grad_tensors([cu(5), cu(4)], cu(3, 5), cu(3, 2, 5)), AssertionError, DIM),
    ("fs.eval_grad_tensors/out-shape", lambda: fs.eval_grad_tensors(T2(), cu(5, 3), cu(3, 2, 5)), TypeError, r"^out: expected a \(3, 5\) torch\.float64 CUDA tensor$"),
    ("fs.eval_grad_tensors/out-rows", lambda: fs.eval_grad_tensors(T2(), cu(3, 10)[:, ::2], cu(3, 2, 5)), ValueError, r"^out: rows must be contiguous$"),
    ("fs.eval_grad_tensors/out-rows-before-grad-shape", lambda: fs.eval_grad_tensors(T2(), cu(3, 10)[:, ::2], cu(3, 2, 6)), ValueError, r"^out: rows must be contiguous$"),
    ("fs.eval_grad_tensors/grad-shape", lambda: fs.eval_grad_tensors(T2(), cu(3, 5), cu(3, 2, 6)), TypeError, r"^grad: expected a \(3, 2, 5\) torch\.float64 CUDA tensor$"),
    ("fs.eval_grad_tensors/grad-dtype", lambda: fs.eval_grad_tensors(T2(), cu(3, 5), cu(3, 2, 5, dtype=F32)), TypeError, r"^grad: expected a \(3, 2, 5\) torch\.float64 CUDA tensor$"),
    ("fs.eval_grad_tensors/grad-last-axis", lambda: fs.eval_grad_tensors(T2(), cu(3, 5), cu(3, 2, 10)[..., ::2]), ValueError, r"^grad: the last axis must be contiguous \(unit stride\)$"),
    ("fs.eval_grad_tensors/grad-uniform", lambda: fs.eval_grad_tensors(T2(), cu(3, 5), cu(3, 3, 5)[:, :2]), ValueError, r"^grad: one uniform stride of at least 5 elements"),
    # ---- Fields: the dispatchers ----
    ("fs.eval_grad/host-takes-no", lambda: fs.eval_grad(O2, z((3, 5)), z((3, 2, 5)), no_alloc=True), TypeError, r"^eval_grad on host arrays takes no \['no_alloc'\]$"),
    ("fs.eval_grad/to-tensors", lambda: fs.eval_grad([cu(5), cu(5, dev=1)], cu(3, 5), cu(3, 2, 5), no_alloc=True), ValueError, r"^obs\[1\]" + LIVES_FS),
    ("fs.eval_points/host-takes-no", lambda: fs.eval_points(z((5, 2)), z((5, 3)), stream=0, no_alloc=True), TypeError, r"^eval_points on a host array takes no \['no_alloc', 'stream'\]$"),
    ("fs.eval_points/to-tensors", lambda: fs.eval_points(cu(5, 2, dev=1), cu(5, 3), stream=0), ValueError, r"^pts" + LIVES_FS),
    ("fs.eval_lattice/host-takes-no", lambda: fs.eval_lattice(A2, z((3, 3, 4)), field_axis=0, stream=0), TypeError, r"^eval_lattice on host arrays takes no \['stream'\]$"),
    ("fs.eval_lattice/host-field-axis", lambda: fs.eval_lattice(A2, z((3, 3, 4)), field_axis=1), ValueError, r"^field_axis: expected 0 \(fields first\) or -1 \(fields last\)$"),
    ("fs.eval_lattice/to-tensors", lambda: fsl.eval_lattice([cu(3), cu(4, dev=1)], cu(3, 3, 4), stream=0), ValueError, r"^axes\[1\]" + LIVES_FS),
    # ---- Fields.eval_points_host ----
    ("fs.eval_points_host/pts-list", lambda: fs.eval_points_host([[0.0, 0.0]], z((1, 3))), TypeError, r"argument 'pts': expected a numpy array, got list"),
    ("fs.eval_points_host/pts-dtype", lambda: fs.eval_points_host(z((5, 2), np.float32), z((5, 3))), TypeError, r"argument 'pts': expected dtype float64, got float32"),
    ("fs.eval_points_host/pts-shape", lambda: fs.eval_points_host(z((5, 3)), z((5, 3))), ValueError, r"^argument 'pts': expected shape \(\.\.\., 2\), got \(5, 3\)$"),
    ("fs.eval_points_host/out-dtype", lambda: fs.eval_points_host(z((5, 2)), z((5, 3), np.float32)), TypeError, r"^out: expected a numpy array of float64$"),
    ("fs.eval_points_host/out-list", lambda: fs.eval_points_host(z((5, 2)), [[0.0] * 3] * 5), TypeError, r"^out: expected a numpy array of float64$"),
    ("fs.eval_points_host/out-shape", lambda: fs.eval_points_host(z((5, 2)), z((5, 2))), ValueError, r"^out: expected shape \(5, 3\), got \(5, 2\)$"),
    ("fs.eval_points_host/out-shape-nd", lambda: fs.eval_points_host(z((2, 3, 2)), z((6, 3))), ValueError, r"^out: expected shape \(2, 3, 3\), got \(6, 3\)$"),
    ("fs.eval_points_host/out-readonly", lambda: fs.eval_points_host(z((5, 2)), ro(5, 3)), ValueError, r"^out: array is read-only$"),
    ("fs.eval_points_host/out-rows", lambda: fs.eval_points_host(z((5, 2)), z((5, 6))[:, ::2]), ValueError, r"^out: every row must be contiguous \(unit stride along the last axis\)$"),
    ("fs.eval_points_host/out-row-stride", lambda: fs.eval_points_host(z((5, 2)), z((5, 3))[::-1]), ValueError, r"^out: the row stride must be a whole number of elements, at least 3$"),
    ("fs.eval_points_host/readonly-before-rows", lambda: fs.eval_points_host(z((5, 2)), ro(5, 6)[:, ::2]), ValueError, r"^out: array is read-only$"),
    ("fs.eval_points_host/out-nd-strided", lambda: fs.eval_points_host(z((2, 3, 2)), z((2, 3, 6))[..., ::2]), ValueError, r"^out: expected a C-contiguous array, or a 2-D array with contiguous rows$"),
    # ---- Fields.eval_points_tensors ----
    ("fs.eval_points_tensors/pts-numpy", lambda: fs.eval_points_tensors(z((5, 2)), cu(5, 3)), TypeError, r"^pts: expected a torch\.float64 CUDA tensor of shape \(\.\.\., 2\)$"),
    ("fs.eval_points_tensors/pts-dtype", lambda: fs.eval_points_tensors(cu(5, 2, dtype=F32), cu(5, 3)), TypeError, r"^pts: expected a torch\.float64 CUDA tensor of shape \(\.\.\., 2\)$"),
    ("fs.eval_points_tensors/pts-shape", lambda: fs.eval_points_tensors(cu(5, 3), cu(5, 3)), ValueError, r"^pts: expected shape \(\.\.\., 2\), got \(5, 3\)$"),
    ("fs.eval_points_tensors/pts-device", lambda: fs.eval_points_tensors(cu(5, 2, dev=1), cu(5, 3)), ValueError, r"^pts" + LIVES_FS),
    ("fs.eval_points_tensors/shape-before-device", lambda: fs.eval_points_tensors(cu(5, 3, dev=1), cu(5, 3)), ValueError, r"^pts: expected shape"),
    ("fs.eval_points_tensors/out-numpy", lambda: fs.eval_points_tensors(cu(5, 2), z((5, 3))), TypeError, r"^out: expected a torch\.float64 CUDA tensor$"),
    ("fs.eval_points_tensors/out-dtype", lambda: fs.eval_points_tensors(cu(5, 2), cu(5, 3, dtype=F32)), TypeError, r"^out: expected a torch\.float64 CUDA tensor$"),
    ("fs.eval_points_tensors/out-shape", lambda: fs.eval_points_tensors(cu(5, 2), cu(5, 2)), ValueError, r"^out: expected shape \(5, 3\), got \(5, 2\)$"),
    ("fs.eval_points_tensors/out-device", lambda: fs.eval_points_tensors(cu(5, 2), cu(5, 3, dev=1)), ValueError, r"^out" + LIVES_FS),
    ("fs.eval_points_tensors/shape-before-out-device", lambda: fs.eval_points_tensors(cu(5, 2), cu(5, 2, dev=1)), ValueError, r"^out: expected shape"),
    ("fs.eval_points_tensors/out-rows", lambda: fs.eval_points_tensors(cu(5, 2), cu(5, 6)[:, ::2]), ValueError, r"^out: every row must be contiguous \(unit stride along the last axis\)$"),
    ("fs.eval_points_tensors/out-row-stride", lambda: fs.eval_points_tensors(cu(5, 2), FakeCuda(torch.zeros(3, dtype=F64).expand(5, 3))), ValueError, r"^out: the row stride must be at least 3$"),
    ("fs.eval_points_tensors/device-before-rows", lambda: fs.eval_points_tensors(cu(5, 2), cu(5, 6, dev=1)[:, ::2]), ValueError, r"^out" + LIVES_FS),
    ("fs.eval_points_tensors/out-nd-strided", lambda: fs.eval_points_tensors(cu(2, 3, 2), cu(2, 3, 6)[..., ::2]), ValueError, r"^out: expected a contiguous tensor, or a 2-D tensor with contiguous rows$"),
    # ---- Fields.eval_lattice_host ----
    ("fs.eval_lattice_host/field-axis", lambda: fs.eval_lattice_host(A2, z((3, 3, 4)), field_axis=1), ValueError, r"^field_axis: expected 0 \(fields first\) or -1 \(fields last\)$"),
    ("fs.eval_lattice_host/field-axis-before-axes", lambda: fs.eval_lattice_host([[0.0]], z((3, 3, 4)), field_axis=2), ValueError, r"^field_axis: expected"),
    ("fs.eval_lattice_host/axes-dtype", lambda: fs.eval_lattice_host([z(3), z(4, np.float32)], z((3, 3, 4))), TypeError, r"argument 'axes\[1\]': expected dtype float64, got float32"),
    ("fs.eval_lattice_host/out-list", lambda: fs.eval_lattice_host(A2, [0.0]), TypeError, r"argument 'out': expected a numpy array, got list"),
    ("fs.eval_lattice_host/out-dtype", lambda: fs.eval_lattice_host(A2, z((3, 3, 4), np.float32)), TypeError, r"argument 'out': expected dtype float64, got float32"),
    ("fs.eval_lattice_host/out-shape", lambda: fs.eval_lattice_host(A2, z((3, 4, 3))), ValueError, r"^out: expected shape \(3, 3, 4\), got \(3, 4, 3\)$"),
    ("fs.eval_lattice_host/out-shape-last", lambda: fs.eval_lattice_host(A2, z((3, 3, 4)), field_axis=-1), ValueError, r"^out: expected shape \(3, 4, 3\), got \(3, 3, 4\)$"),
    ("fs.eval_lattice_host/out-block", lambda: fs.eval_lattice_host(A2, z((3, 3, 8))[..., ::2]), ValueError, r"^out: each field's block must be contiguous$"),
    ("fs.eval_lattice_host/out-readonly", lambda: fs.eval_lattice_host(A2, ro(3, 3, 4)), ValueError, r"argument 'out': array is read-only"),
    ("fs.eval_lattice_host/layout-before-readonly", lambda: fs.eval_lattice_host(A2, ro(3, 3, 8)[..., ::2]), ValueError, r"^out: each field's block"),
    # ---- Fields.eval_lattice_tensors ----
    ("fs.eval_lattice_tensors/field-axis", lambda: fsl.eval_lattice_tensors(TA2(), cu(3, 3, 4), field_axis=1), ValueError, r"^field_axis: expected 0 \(fields first\) or -1 \(fields last\)$"),
    ("fs.eval_lattice_tensors/axes-numpy", lambda: fsl.eval_lattice_tensors(A2, cu(3, 3, 4)), TypeError, r"^axes\[0\]: " + CONTIG_1D),
    ("fs.eval_lattice_tensors/axes-device", lambda: fsl.eval_lattice_tensors([cu(3), cu(4, dev=1)], cu(3, 3, 4)), ValueError, r"^axes\[1\]" + LIVES_FS),
    ("fs.eval_lattice_tensors/out-numpy", lambda: fsl.eval_lattice_tensors(TA2(), z((3, 3, 4))), TypeError, r"^out: expected a torch\.float64 CUDA tensor$"),
    ("fs.eval_lattice_tensors/out-dtype", lambda: fsl.eval_lattice_tensors(TA2(), cu(3, 3, 4, dtype=F32)), TypeError, r"^out: expected a torch\.float64 CUDA tensor$"),
    ("fs.eval_lattice_tensors/out-device", lambda: fsl.eval_lattice_tensors(TA2(), cu(3, 3, 4, dev=1)), ValueError, r"^out" + LIVES_FS),
    ("fs.eval_lattice_tensors/out-shape", lambda: fsl.eval_lattice_tensors(TA2(), cu(3, 4, 3)), ValueError, r"^out: expected shape \(3, 3, 4\), got \(3, 4, 3\)$"),
    ("fs.eval_lattice_tensors/device-before-shape", lambda: fsl.eval_lattice_tensors(TA2(), cu(3, 4, 3, dev=1)), ValueError, r"^out" + LIVES_FS),
    ("fs.eval_lattice_tensors/out-rows-last", lambda: fsl.eval_lattice_tensors(TA2(), cu(12, 6)[:, ::2], field_axis=-1), ValueError, r"^out: every row must be contiguous \(unit stride along the last axis\)$"),

    # ---- the helpers ----
    ("interpn/dtype", lambda: interpn_amd.interpn(OB, G, V.astype(np.int32)), AssertionError, F3264),
    ("interpn/method", lambda: interpn_amd.interpn(OB, G, V, method="quintic"), ValueError, r"^Unsupported interpolation configuration: float64, False, quintic$"),
    ("_interpn_on_device/method", lambda: interpn_amd._interpn_on_device([cu(6), cu(6)], G, V, "quintic", None, True, False, False, 1e-8), ValueError, r"^Unsupported interpolation configuration: quintic$"),
    ("_interpn_on_device/dtype", lambda: interpn_amd._interpn_on_device([cu(6), cu(6)], G, V.astype(np.int32), "linear", None, True, False, False, 1e-8), AssertionError, F3264),
    ("interpn_grad/method", lambda: interpn_amd.interpn_grad(OB, G, V, method="nearest"), ValueError, r"^interpn_grad: method must be \"linear\" or \"cubic\", got 'nearest'$"),
    ("interpn_grad/method-before-vals", lambda: interpn_amd.interpn_grad(OB, G, [0.0], method="quintic"), ValueError, r"^interpn_grad: method must be"),
    ("interpn_grad/vals-list", lambda: interpn_amd.interpn_grad(OB, G, V.tolist()), TypeError, r"^argument 'vals': expected a numpy array or a torch tensor$"),
    ("interpn_grad/vals-cpu-tensor", lambda: interpn_amd.interpn_grad(OB, G, torch.zeros(4, 5, dtype=F64)), TypeError, r"^argument 'vals': expected a numpy array or a torch tensor$"),
    ("interpn_grad/dtype", lambda: interpn_amd.interpn_grad(OB, G, V.astype(np.int64)), AssertionError, F3264),
    ("interpn_points/method", lambda: interpn_amd.interpn_points(XI, G, V, method="quintic"), ValueError, r"^Unsupported interpolation configuration: quintic$"),
    ("interpn_points/xi-width", lambda: interpn_amd.interpn_points(z((6, 3)), G, V), AssertionError, DIM),
    ("interpn_points/xi-0d", lambda: interpn_amd.interpn_points(0.5, G, V), AssertionError, DIM),
    ("interpn_points/xi-before-vals", lambda: interpn_amd.interpn_points(z((6, 3)), G, V.tolist()), AssertionError, DIM),
    ("interpn_points/method-before-xi", lambda: interpn_amd.interpn_points(z((6, 3)), G, V, method="quintic"), ValueError, r"^Unsupported"),
    ("interpn_points/vals-list", lambda: interpn_amd.interpn_points(XI, G, V.tolist()), TypeError, r"^argument 'vals': expected a numpy array or a torch tensor$"),
    ("interpn_points/dtype", lambda: interpn_amd.interpn_points(XI, G, V.astype(np.int32)), AssertionError, F3264),
    ("interpn_points_grad/method", lambda: interpn_amd.interpn_points_grad(XI, G, V, method="nearest"), ValueError, r"^interpn_points_grad: method must be \"linear\" or \"cubic\", got 'nearest'$"),
    ("interpn_points_grad/xi-width", lambda: interpn_amd.interpn_points_grad(z((6, 3)), G, V), AssertionError, DIM),
    ("interpn_points_grad/xi-before-vals", lambda: interpn_amd.interpn_points_grad(z((6, 3)), G, None), AssertionError, DIM),
    ("interpn_points_grad/vals-list", lambda: interpn_amd.interpn_points_grad(XI, G, V.tolist()), TypeError, r"^argument 'vals': expected a numpy array or a torch tensor$"),
    ("interpn_points_grad/dtype", lambda: interpn_amd.interpn_points_grad(XI, G, V.astype(np.int32)), AssertionError, F3264),
    ("interpn_lattice/method", lambda: interpn_amd.interpn_lattice(AX, G, V, method="quintic"), ValueError, r"^Unsupported interpolation configuration: quintic$"),
    ("interpn_lattice/axes-count", lambda: interpn_amd.interpn_lattice(AX[:1], G, V), ValueError, r"^axes: expected 2 coordinate vectors \(one per grid axis\), got 1$"),
    ("interpn_lattice/axes-before-vals", lambda: interpn_amd.interpn_lattice(AX[:1], G, V.tolist()), ValueError, r"^axes: expected 2 coordinate vectors"),
    ("interpn_lattice/vals-list", lambda: interpn_amd.interpn_lattice(AX, G, V.tolist()), TypeError, r"^argument 'vals': expected a numpy array or a torch tensor$"),
    ("interpn_lattice/dtype", lambda: interpn_amd.interpn_lattice(AX, G, V.astype(np.int32)), AssertionError, F3264),
    ("interpn_lattice/out-shape", lambda: interpn_amd.interpn_lattice(AX, G, V, out=z((6, 3))), ValueError, r"^out: expected shape \(3, 6\), got \(6, 3\)$"),
    ("interpn_lattice/dtype-before-out", lambda: interpn_amd.interpn_lattice(AX, G, V.astype(np.int32), out=z((6, 3))), AssertionError, F3264),
    ("interpn_fields/field-axis", lambda: interpn_amd.interpn_fields(OB, G, VK, field_axis=1), ValueError, r"^field_axis: expected 0 \(fields first\) or -1 \(fields last\)$"),
    ("interpn_fields/field-axis-before-method", lambda: interpn_amd.interpn_fields(OB, G, VK, field_axis=1, method="quintic"), ValueError, r"^field_axis: expected"),
    ("interpn_fields/method", lambda: interpn_amd.interpn_fields(OB, G, VK, method="quintic"), ValueError, r"^Unsupported interpolation configuration: quintic$"),
    ("interpn_fields/method-before-vals", lambda: interpn_amd.interpn_fields(OB, G, None, method="quintic"), ValueError, r"^Unsupported"),
    ("interpn_fields/vals-list", lambda: interpn_amd.interpn_fields(OB, G, VK.tolist()), TypeError, r"^vals: expected a numpy array or a torch tensor with a field axis$"),
    ("interpn_fields/dtype", lambda: interpn_amd.interpn_fields(OB, G, VK.astype(np.int32)), AssertionError, F3264),
    ("interpn_fields/vals-1d", lambda: interpn_amd.interpn_fields(OB, G, z(60)), ValueError, r"^vals: expected a field axis besides the grid's values$"),
    ("interpn_fields/vals-count", lambda: interpn_amd.interpn_fields(OB, G, z((3, 4, 4))), ValueError, r"^vals: expected 3 x 20 values for grids of \[4, 5\], got shape \(3, 4, 4\)$"),
    ("interpn_fields/vals-count-last", lambda: interpn_amd.interpn_fields(OB, G, z((4, 4, 3)), field_axis=-1), ValueError, r"^vals: expected 3 x 20 values for grids of \[4, 5\], got shape \(4, 4, 3\)$"),
    ("interpn_fields/out-shape", lambda: interpn_amd.interpn_fields(OB, G, VK, out=z((6, 3))), ValueError, r"^out: expected shape \(3, 6\), got \(6, 3\)$"),
    ("interpn_fields/out-shape-last", lambda: interpn_amd.interpn_fields(OB, G, VL, field_axis=-1, out=z((3, 6))), ValueError, r"^out: expected shape \(6, 3\), got \(3, 6\)$"),
    ("interpn_fields/vals-count-before-out", lambda: interpn_amd.interpn_fields(OB, G, z((3, 4, 4)), out=z((6, 3))), ValueError, r"^vals: expected 3 x 20"),
    ("interpn_fields_grad/field-axis", lambda: interpn_amd.interpn_fields_grad(OB, G, VK, field_axis=2), ValueError, r"^field_axis: expected 0 \(fields first\) or -1 \(fields last\)$"),
    ("interpn_fields_grad/method", lambda: interpn_amd.interpn_fields_grad(OB, G, VK, method="quintic"), ValueError, r"^Unsupported interpolation configuration: quintic$"),
    ("interpn_fields_grad/vals-list", lambda: interpn_amd.interpn_fields_grad(OB, G, VK.tolist()), TypeError, r"^vals: expected a numpy array or a torch tensor with a field axis$"),
    ("interpn_fields_grad/dtype", lambda: interpn_amd.interpn_fields_grad(OB, G, VK.astype(np.int32)), AssertionError, F3264),
    ("interpn_fields_grad/vals-1d", lambda: interpn_amd.interpn_fields_grad(OB, G, z(60)), ValueError, r"^vals: expected a field axis besides the grid's values$"),
    ("interpn_fields_grad/vals-count", lambda: interpn_amd.interpn_fields_grad(OB, G, z((3, 5, 5))), ValueError, r"^vals: expected 3 x 20 values for grids of \[4, 5\], got shape \(3, 5, 5\)$"),
    ("interpn_fields_lattice/field-axis", lambda: interpn_amd.interpn_fields_lattice(AX, G, VK, field_axis=1), ValueError, r"^field_axis: expected 0 \(fields first\) or -1 \(fields last\)$"),
    ("interpn_fields_lattice/method", lambda: interpn_amd.interpn_fields_lattice(AX, G, VK, method="quintic"), ValueError, r"^Unsupported interpolation configuration: quintic$"),
    ("interpn_fields_lattice/vals-list", lambda: interpn_amd.interpn_fields_lattice(AX, G, VK.tolist()), TypeError, r"^vals: expected a numpy array or a torch tensor with a field axis$"),
    ("interpn_fields_lattice/dtype", lambda: interpn_amd.interpn_fields_lattice(AX, G, VK.astype(np.int32)), AssertionError, F3264),
    ("interpn_fields_lattice/vals-1d", lambda: interpn_amd.interpn_fields_lattice(AX, G, z(60)), ValueError, r"^vals: expected a field axis besides the grid's values$"),
    ("interpn_fields_lattice/vals-1d-before-axes", lambda: interpn_amd.interpn_fields_lattice(AX[:1], G, z(60)), ValueError, r"^vals: expected a field axis"),
    ("interpn_fields_lattice/axes-count", lambda: interpn_amd.interpn_fields_lattice(AX[:1], G, VK), ValueError, r"^axes: expected 2 coordinate vectors \(one per grid axis\), got 1$"),
    ("interpn_fields_lattice/axes-before-vals-count", lambda: interpn_amd.interpn_fields_lattice(AX[:1], G, z((3, 4, 4))), ValueError, r"^axes: expected 2 coordinate vectors"),
    ("interpn_fields_lattice/vals-count", lambda: interpn_amd.interpn_fields_lattice(AX, G, z((3, 4, 4))), ValueError, r"^vals: expected 3 x 20 values for grids of \[4, 5\], got shape \(3, 4, 4\)$"),
    ("interpn_fields_lattice/out-shape", lambda: interpn_amd.interpn_fields_lattice(AX, G, VK, out=z((3, 6, 3))), ValueError, r"^out: expected shape \(3, 3, 6\), got \(3, 6, 3\)$"),
    ("interpn_fields_lattice/out-shape-last", lambda: interpn_amd.interpn_fields_lattice(AX, G, VL, field_axis=-1, out=z((3, 3, 6))), ValueError, r"^out: expected shape \(3, 6, 3\), got \(3, 3, 6\)$"),
    ("interpn_fields_points/method", lambda: interpn_amd.interpn_fields_points(XI, G, VL, method="quintic"), ValueError, r"^Unsupported interpolation configuration: quintic$"),
    ("interpn_fields_points/vals-list", lambda: interpn_amd.interpn_fields_points(XI, G, VL.tolist()), TypeError, r"^vals: expected a numpy array or a torch tensor with a trailing field axis$"),
    ("interpn_fields_points/dtype", lambda: interpn_amd.interpn_fields_points(XI, G, VL.astype(np.int32)), AssertionError, F3264),
    ("interpn_fields_points/xi-list", lambda: interpn_amd.interpn_fields_points(XI.tolist(), G, VL), TypeError, r"^xi: expected a numpy array or a torch tensor of shape \(\.\.\., N\)$"),
    ("interpn_fields_points/dtype-before-xi", lambda: interpn_amd.interpn_fields_points(XI.tolist(), G, VL.astype(np.int32)), AssertionError, F3264),
    ("interpn_fields_points/vals-shape", lambda: interpn_amd.interpn_fields_points(XI, G, V), ValueError, r"^vals: expected shape \(\*dims, K\) for 2 grids, got \(4, 5\)$"),
    ("interpn_fields_points/xi-shape", lambda: interpn_amd.interpn_fields_points(z((6, 3)), G, VL), ValueError, r"^xi: expected shape \(\.\.\., 2\), got \(6, 3\)$"),
    ("interpn_fields_points/vals-shape-before-xi", lambda: interpn_amd.interpn_fields_points(z((6, 3)), G, V), ValueError, r"^vals: expected shape"),
    ("interpn_fields_points/vals-dims", lambda: interpn_amd.interpn_fields_points(XI, G, z((4, 4, 3))), ValueError, r"^vals: expected 3 x 20 values for grids of \[4, 5\], got shape \(4, 4, 3\)$"),
    ("interpn_fields_points/xi-dtype", lambda: interpn_amd.interpn_fields_points(XI.astype(np.float32), G, VL), TypeError, r"^xi: expected dtype float64 \(that of vals\), got float32$"),
    ("interpn_fields_points/xi-dtype-before-out", lambda: interpn_amd.interpn_fields_points(XI.astype(np.float32), G, VL, out=z((3, 6))), TypeError, r"^xi: expected dtype"),
    ("interpn_fields_points/out-shape", lambda: interpn_amd.interpn_fields_points(XI, G, VL, out=z((3, 6))), ValueError, r"^out: expected shape \(6, 3\), got \(3, 6\)$"),
    ("interpn_fields_points/xi-cpu-tensor", lambda: interpn_amd.interpn_fields_points(torch.zeros(6, 2, dtype=F64), G, VL), TypeError, r"^xi: expected a numpy array or a torch CUDA tensor$"),
    ("interpn_fields_points/out-before-cpu-tensor", lambda: interpn_amd.interpn_fields_points(torch.zeros(6, 2, dtype=F64), G, VL, out=z((3, 6))), ValueError, r"^out: expected shape"),
]

# The one intended difference from the code these rows were first written against: the four methods below used to look
# at `.is_cuda` unguarded, so an object without it (a numpy array) raised AttributeError; now they raise what their
# siblings always raised.
ROWS += [
    ("it.eval_tensors/obs-numpy", lambda: it.eval_tensors(O3, cu(5)), TypeError, r"^obs\[0\]: " + CONTIG_1D),
    ("it.check_bounds_tensors/obs-numpy", lambda: it.check_bounds_tensors(O3, 1e-8), TypeError, r"^obs\[0\]: " + CONTIG_1D),
    ("fs.eval_tensors/obs-numpy", lambda: fs.eval_tensors(O2, cu(3, 5)), TypeError, r"^obs\[0\]: " + CONTIG_1D),
    ("fs.eval_grad_tensors/obs-numpy", lambda: fs.eval_grad_tensors(O2, cu(3, 5), cu(3, 2, 5)), TypeError, r"^obs\[0\]: " + CONTIG_1D),
]


def test_the_rows_have_distinct_names():
    names = [r[0] for r in ROWS]
    assert len(set(names)) == len(names)


@pytest.mark.parametrize("call, exc, pattern", [pytest.param(*r[1:], id=r[0]) for r in ROWS])
def test_malformed_call(call, exc, pattern):
    with pytest.raises(exc, match=pattern) as info:
        call()
    assert type(info.value) is exc, type(info.value)
