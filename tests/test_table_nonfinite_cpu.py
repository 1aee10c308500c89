"""Tables with NaN and ±inf nodes, on the CPU: the oracle's contract, which tests/test_table_nonfinite_gpu.py holds every
value kernel to.  A non-finite node makes the result non-finite at exactly the points whose arithmetic touches it (a weight
of 0 still counts: 0 · NaN = NaN), and every other point keeps the bits it has on the clean table.  Which points touch a
node is the footprint rule of tests/helpers.py::footprint_poisoned, written with numpy and sharing no code with oracle/;
here the oracle is shown to follow it exactly, so that on the GPU the rule and the oracle are two independent witnesses.

Tables are those of `anisotropic_case` (every finite node U(-1, 1)) poisoned by tests/helpers.py::poison_table: "nan" and
"mixed" (NaN / +inf / -inf) at a share of the nodes that leaves about half the points clean, and "plane" (one whole
hyperplane, index 3 of the longest axis) for the runs the GPU file makes on such tables."""

import numpy as np
import pytest

from tests import family_runs as fr
from tests.helpers import footprint_cells, footprint_poisoned, poison_count, poison_table, run_oracle

LINEAR = [[9, 7], [6, 5, 7], [5, 6, 4, 5], [4, 3, 5, 3, 4], [3, 4, 2, 5, 3, 4], [70, 9, 7], [20, 17, 33], [24, 11, 40], [70, 90],
          [2, 3, 2, 3, 2, 3, 2]]
CUBIC = [[9, 7], [6, 5, 7], [5, 6, 4, 5], [70, 9, 7], [20, 17, 33], [150, 140], [8, 70, 90], [4, 5, 4, 5, 4]]
FLAVOURS = [("linear", False, s) for s in LINEAR] + [("cubic", lin, s) for lin in (False, True) for s in CUBIC]
NPTS = 2001


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
@pytest.mark.parametrize("method,linearize,shape", FLAVOURS,
                         ids=[f"{m}{'_lin' if lin else ''}-{'x'.join(map(str, s))}" for m, lin, s in FLAVOURS])
def test_oracle_follows_the_footprint_rule(oracle, method, linearize, shape, kind, dtype):
    """Both fma flavours, the "nan" and the "mixed" table.  No point is excluded: the comparison is over all 2001 points, exact
    nodes and the ends' floating-point neighbours among them."""
    clean = fr.make_case(method, kind, shape, dtype, nobs=NPTS, linearize=linearize)
    assert np.isfinite(clean.vals).all() and np.abs(clean.vals).max() <= 1
    for table in ("nan", "mixed"):
        case = fr.poisoned_case(clean, table)
        bad = ~np.isfinite(case.vals)
        assert bad.sum() == poison_count(shape, method) and np.array_equal(case.vals[~bad], clean.vals[~bad])
        if table == "nan":
            assert np.isnan(case.vals[bad]).all()
        touched = footprint_poisoned(case)
        assert 0.25 <= touched.mean() <= 0.75, float(touched.mean())
        for fma in (True, False):
            got, base = run_oracle(oracle, case, fma), run_oracle(oracle, clean, fma)
            assert np.isfinite(base).all()
            assert np.array_equal(~np.isfinite(got), touched), (table, fma, int((~np.isfinite(got) != touched).sum()))
            assert np.array_equal(fr.bits(got)[~touched], fr.bits(base)[~touched]), (table, fma)
            assert 0.25 <= (~np.isfinite(got)).mean() <= 0.75


@pytest.mark.parametrize("row", list(fr.plane_cases()), ids=fr.plane_id)
def test_plane_tables(oracle, row):
    """The "plane" runs of the GPU file (f64, fma): every node with index 3 along the longest axis is NaN.  The oracle
    follows the rule, at least 20 points stay finite and at least 20 do not, and the points in that axis's first cell or
    below the grid are among the finite ones — for multicubic node 3 is the fourth node of the saturated cell, computed by
    `cubic_rect_node_fast` and dropped by a select."""
    family, sub, method, kind, shape, nobs, linearize = row
    clean = fr.make_case(method, kind, shape, np.float64, nobs=nobs, linearize=linearize)
    case = fr.poisoned_case(clean, "plane")
    d = int(np.argmax(shape))
    assert shape[d] >= 5 and np.isnan(case.vals).sum() == case.vals.size // shape[d]
    assert np.isnan(case.vals.reshape(shape).take(3, axis=d)).all()
    got, base = run_oracle(oracle, case, True), run_oracle(oracle, clean, True)
    touched = footprint_poisoned(case)
    assert np.array_equal(~np.isfinite(got), touched)
    assert np.array_equal(fr.bits(got)[~touched], fr.bits(base)[~touched])
    assert np.isfinite(got).sum() >= 20 and (~np.isfinite(got)).sum() >= 20
    first = footprint_cells(case)[d] == 0
    assert first.sum() >= 10 and (case.obs[d][first] < case.grids[d][0]).any() and np.isfinite(got[first]).all()


def test_poison_table_and_the_rule_by_hand():
    """The helpers on a table small enough to check by hand: 1-D, 6 nodes at 0 .. 5, node 3 poisoned."""
    from tests.kat import Case

    g = np.arange(6.0)
    x = np.array([-1.0, 0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0, 4.5, 5.0, 7.0])
    vals = np.arange(6.0)
    vals[3] = np.inf
    for kind in ("regular", "rectilinear"):
        lin = Case("hand", "linear", kind, [g], vals, [x], np.zeros(x.size), 0.0)
        cub = Case("hand", "cubic", kind, [g], vals, [x], np.zeros(x.size), 0.0)
        # a coordinate on a node belongs to the cell that starts there (regular) or ends there (rectilinear)
        cells = [0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 4, 4] if kind == "regular" else [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 4]
        assert footprint_cells(lin)[0].tolist() == cells
        assert footprint_poisoned(lin).tolist() == [c in (2, 3) for c in cells]       # nodes c, c + 1
        assert footprint_poisoned(cub).tolist() == [c in (1, 2, 3, 4) for c in cells]  # cell 0 uses 0 .. 2 only
    v = np.linspace(-1, 1, 5 * 6 * 4)
    p = poison_table(v, [5, 6, 4], "linear", 1, "plane")
    assert np.array_equal(np.isnan(p.reshape(5, 6, 4)), np.arange(6)[None, :, None] == np.full((5, 1, 4), 3))
    m = poison_table(v, [5, 6, 4], "cubic", 1, "mixed")
    assert (~np.isfinite(m)).sum() == poison_count([5, 6, 4], "cubic") == 1 and np.isfinite(v).all()
    n = poison_table(v, [5, 6, 4], "nearest", 1, "nan")
    assert np.isnan(n).sum() == 60 and np.array_equal(np.isnan(n), np.isnan(poison_table(v, [5, 6, 4], "nearest", 1, "nan")))
