"""The table of the reference's fused multiply-add sites (tests/golden/fma_sites.json), checked mechanically, and the k1
probe that is driven by it.

The oracle and the kernels were written by one reader from the same lines of the reference, so a site read wrong in both
places passes every parity test.  Two things here do not depend on that reader:

  the table    one row per line of the reference that says `mul_add` (the frozen index tests/golden/reference_citations.json
               knows which lines those are), plus the sites that stay unfused under `fma` although their twin in the other
               arm or class is fused.  Every row names the functions that implement the site, and each of them must cite
               the row's module path and line — so a site that the table lists and a function does not know of shows here.
  the probe    tables on which 2 dy overflows in an end cell while 2 dy - k0 does not (tests/helpers.py::k1_probe_case):
               there `two.mul_add(dy, -k0)` is finite and `two * dy - k0` is not, so the oracle's result says which form a
               class took.  What it must be — finite, or not — is read from the table per (grid kind, arm, class), and
               where it is finite it is compared with oracle/exact_rational.py, which shares no code with the oracle."""
import ast
import json
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from oracle import exact_rational
from tests.helpers import K1_CLASSES, K1_MIDDLE, fma_sites, k1_expected_fused as expected_fused, k1_probe_case, run_oracle
from tests.test_golden import EXACT_K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

SITES = fma_sites()
with open(os.path.join(GOLDEN, "reference_citations.json")) as _f:
    INDEX = json.load(_f)["files"]

ROWS = [("fused", r) for r in SITES["fused"]] + [("unfused", r) for r in SITES["unfused"]]
ROW_IDS = [f"{s}-{r['file'][4:]}:{r['line']}" for s, r in ROWS]

# `module/file.rs:L`, and what follows it of `, :L` / ` / :L` / ` and :L` (further lines of the same file)
SITE_CITE = re.compile(r"((?:src/)?(?:[a-z_]+/)+[a-z_]+\.rs):(\d+)(-\d+)?((?:\s*(?:,|/|and)\s*:\d+(?:-\d+)?)*)")


def single_line_citations(text):
    """{(path under src/, line)} of the citations in `text` that carry a module path and name ONE line (a range is no
    citation of a site)."""
    out = set()
    for m in SITE_CITE.finditer(text):
        path = m.group(1)[4:] if m.group(1).startswith("src/") else m.group(1)
        if not m.group(3):
            out.add((path, int(m.group(2))))
        for more in re.finditer(r":(\d+)(-\d+)?", m.group(4)):
            if not more.group(2):
                out.add((path, int(more.group(1))))
    return out


def _matching(text, at, opening, closing):
    depth = 0
    for k in range(at, len(text)):
        if text[k] == opening:
            depth += 1
        elif text[k] == closing:
            depth -= 1
            if depth == 0:
                return k
    raise AssertionError("unbalanced")


def function_text(spec):
    """The text of `path::name`: a Python function (its def through its last line), or in C++ the body of the function
    `name` or of the primary template `struct name` — from the name to the closing brace.  None if there is none."""
    path, name = spec.split("::")
    with open(os.path.join(ROOT, path)) as f:
        text = f.read()
    if path.endswith(".py"):
        for node in ast.walk(ast.parse(text)):
            if isinstance(node, ast.FunctionDef) and node.name == name:
                return "\n".join(text.split("\n")[node.lineno - 1:node.end_lineno])
        return None
    m = re.search(r"\bstruct\s+" + name + r"\s*\{", text)
    if m:
        return text[m.start():_matching(text, m.end() - 1, "{", "}") + 1]
    # a definition: `name(` right after a type (a call of a template names its arguments, `name<...>(`), the parameter list,
    # then the body
    for m in re.finditer(r"[\w>&*)]\s+" + name + r"\(", text):
        close = _matching(text, m.end() - 1, "(", ")")
        rest = re.match(r"\s*(?:const\s*)?\{", text[close + 1:])
        if rest:
            return text[m.start():_matching(text, close + rest.end(), "{", "}") + 1]
    return None


def test_fused_rows_are_the_mul_add_lines_of_the_frozen_index():
    want = {(path, ln) for path, rec in INDEX.items() for ln in rec["mul_add_lines"]}
    rows = [(r["file"], r["line"]) for r in SITES["fused"]]
    assert len(rows) == len(set(rows)) == 27, len(rows)
    assert set(rows) == want, (sorted(set(rows) - want), sorted(want - set(rows)))


def test_unfused_rows_are_lines_that_do_not_fuse_and_name_a_fused_twin():
    fused = {f"{r['file']}:{r['line']}" for r in SITES["fused"]}
    rows = [(r["file"], r["line"]) for r in SITES["unfused"]]
    assert len(rows) == len(set(rows)) == 9, len(rows)
    for r in SITES["unfused"]:
        rec = INDEX[r["file"]]
        assert 1 <= r["line"] <= rec["lines"] and r["line"] not in rec["mul_add_lines"], (r["file"], r["line"])
        assert r["fused_twin"] in fused, r["fused_twin"]
    # the sites the flattened rectilinear multicubic arm never fuses, and the three the recursive arms keep unfused
    assert {(f, ln) for f, ln in rows if f == "src/multicubic/rectilinear.rs"} == {("src/multicubic/rectilinear.rs", ln) for ln in (471, 493, 500, 515, 532, 539)}
    assert {(f[15:], ln) for f, ln in rows if f != "src/multicubic/rectilinear.rs"} == {("regular_recursive.rs", 536), ("rectilinear_recursive.rs", 469), ("rectilinear_recursive.rs", 519)}


@pytest.mark.parametrize("status,row", ROWS, ids=ROW_IDS)
def test_row_is_complete_and_every_function_it_names_cites_it(status, row):
    assert set(row) >= {"file", "line", "arm", "method", "kind", "n", "label", "functions"}, sorted(row)
    assert row["file"] in INDEX and row["file"].startswith("src/")
    assert row["arm"] in ("flattened", "recursive", "shared") and row["kind"] in ("regular", "rectilinear", "both")
    assert row["method"] in ("linear", "cubic", "nearest", "Linear1D", "LinearHoldLast1D")
    lo, hi = row["n"]
    assert 1 <= lo <= hi <= 8
    assert ("recursive" in row["file"]) == (row["arm"] == "recursive"), (row["file"], row["arm"])
    assert row["label"] and "mul_add" not in row["label"]
    assert len(row["functions"]) >= 2, row["functions"]
    assert any(f.startswith("interpn_amd/csrc/") for f in row["functions"]), "no device function"
    site = (row["file"][4:], row["line"])
    for spec in row["functions"]:
        text = function_text(spec)
        assert text is not None, f"{spec} does not exist"
        assert site in single_line_citations(text), f"{spec} does not cite {site[0]}:{site[1]}"


def test_function_text_finds_bodies_not_calls():
    """The finder itself: a definition, not a call or a specialisation; the whole body; None for a name that is not there."""
    node = function_text("interpn_amd/csrc/interpn_device.h::cubic_rect_node")
    assert node.rstrip().endswith("}") and "cubic_rect_saturated<FMA, T>(v0, v1, v2, v3, d, y0, y1, dy, k0);" in node
    assert "cubic_rect_node_fast" not in node and "return hermite<FMA>(d.t, y0, dy, k0, k1);" in node
    tree = function_text("interpn_amd/csrc/interpn_device.h::LinearTree")
    assert "mul_add<FMA>(t[D - 1], dy, y0)" in tree and "load_leaf" not in tree
    assert "def combine" in function_text("tests/cubic_grad_restatement.py::node")
    assert function_text("interpn_amd/csrc/interpn_device.h::no_such_function") is None
    assert function_text("tests/cubic_grad_restatement.py::no_such_function") is None
    assert single_line_citations("// multicubic/regular.rs:560, :616, multicubic/regular_recursive.rs:547 and :603, regular.rs:528, "
                                 "multicubic/mod.rs:72-91 / :89") == {("multicubic/regular.rs", 560), ("multicubic/regular.rs", 616),
                                                                      ("multicubic/regular_recursive.rs", 547),
                                                                      ("multicubic/regular_recursive.rs", 603), ("multicubic/mod.rs", 89)}


def test_frozen_index_matches_the_reference_tree():
    """tests/golden/make_citation_index.py regenerated in memory where the reference tree is at hand (INTERPN_REFERENCE_TREE,
    or a directory `reference` beside the repository); elsewhere the frozen index is all there is."""
    tree = os.environ.get("INTERPN_REFERENCE_TREE") or os.path.join(os.path.dirname(ROOT), "reference")
    if not os.path.isdir(os.path.join(tree, "src", "multicubic")):
        pytest.skip("no reference tree here")
    from tests.golden.make_citation_index import index

    assert index(tree) == INDEX


# ---- the k1 probe ----------------------------------------------------------------------------------------------------------------------
PROBE_SHAPES = {3: [4, 5, 4], 5: [4, 5, 4, 5, 4]}


def test_table_gives_the_four_patterns_of_the_two_arms():
    got = {(kind, n): [K1_CLASSES[c] for c in range(4) if expected_fused(kind, n, c)] for kind in ("regular", "rectilinear") for n in (3, 5)}
    assert got == {("regular", 3): list(K1_CLASSES), ("regular", 5): ["InsideLow", "InsideHigh", "OutsideHigh"],
                   ("rectilinear", 3): [], ("rectilinear", 5): ["InsideLow", "InsideHigh"]}


def _exact_along_axis(case, axis):
    """(value, bound scale) per point from oracle/exact_rational.py::evaluate_with_condition on the 1-D problem of `axis`: the
    table varies along that axis only and the interpolant reproduces constants along every other, so the N-D value IS the
    1-D value; the N-D bound scale is at least the 1-D one (the other axes add sum |w| >= 1 as factors and no derivative
    term), so the 1-D scale gives the stricter bound."""
    index = [0] * len(case.dims)
    index[axis] = slice(None)
    profile = case.vals.reshape(case.dims)[tuple(index)]
    kw = dict(starts=[case.starts[axis]], steps=[case.steps[axis]]) if case.kind == "regular" else {}
    return exact_rational.evaluate_with_condition("cubic", case.kind, [case.grids[axis]], profile, [case.obs[axis]],
                                                  linearize=case.linearize, **kw)


def _probe(oracle, kind, n, dtype, fma, linearize):
    """Runs the probe over every axis in the role of the varying one.  Returns the largest error of a fused-class or
    middle-cell result against the exact value, in units of u * (1-D bound scale) and of eps * max."""
    info = np.finfo(dtype)
    top, u = Fraction(float(info.max)), Fraction(float(info.eps)) / 2
    worst_scale = worst_max = Fraction(0)
    shape = PROBE_SHAPES[n]
    for axis in range(n):
        case, cls = k1_probe_case(kind, shape, axis, dtype, linearize=linearize)
        with np.errstate(all="ignore"):
            got = run_oracle(oracle, case, fma)
        exact = _exact_along_axis(case, axis)
        for c in range(5):
            at = np.flatnonzero(cls == c)
            assert at.size >= 24
            what = (kind, n, np.dtype(dtype).name, "fma" if fma else "nofma", linearize, axis, "middle" if c == K1_MIDDLE else K1_CLASSES[c])
            # the inputs themselves: the exact value is representable at every point, so a non-finite result is the form's doing
            assert all(abs(exact[i][0]) < top for i in at), what
            finite = c == K1_MIDDLE or (fma and expected_fused(kind, n, c))
            if not finite:
                assert not np.isfinite(got[at]).any(), (what, "finite results where 2 dy overflows unfused", int(np.isfinite(got[at]).sum()))
                continue
            assert np.isfinite(got[at]).all(), (what, "non-finite results", int((~np.isfinite(got[at])).sum()))
            for i in at:
                val, scale = exact[i]
                err = abs(Fraction(float(got[i])) - val)
                assert err <= Fraction(EXACT_K) * u * scale, (what, int(i), float(err / (u * scale)))
                worst_scale = max(worst_scale, err / (u * scale))
                worst_max = max(worst_max, err / (Fraction(float(info.eps)) * top))
    return float(worst_scale), float(worst_max)


@pytest.mark.parametrize("linearize", [False, True], ids=["quad", "lin"])
@pytest.mark.parametrize("fma", [True, False], ids=["fma", "nofma"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n", [3, 5], ids=["N3", "N5"])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_k1_probe_oracle_is_finite_exactly_where_the_table_says_fused(oracle, kind, n, dtype, fma, linearize):
    """Per (grid kind, arm, class): where the table says fused the oracle under `fma` is finite and within the bound of
    tests/test_golden.py (EXACT_K * u * scale) of the exact value; where it says unfused, and everywhere without `fma`, every
    result is non-finite; the middle cells are finite in both flavours.  (An Outside class with linearize_extrapolation returns
    k1 (t - 1) + y1: k1 is what the class's row says, and an infinite k1 gives an infinite result there too.)

    Measured on these inputs, the oracle's largest error where it is finite: 0.80 u * scale for f64 and 0.62 u * scale for f32
    (bound: 16), which is 1.1 eps * max (f64) and 1.2 eps * max (f32) — the bound of tests/test_golden.py fits these
    magnitudes, so it is the one asserted."""
    _probe(oracle, kind, n, dtype, fma, linearize)


def test_k1_probe_reduction_to_one_axis_is_the_n_dimensional_exact_value():
    """What _exact_along_axis relies on, checked on the full tensor-product evaluation (oracle/exact_rational.py::evaluate)
    for a few points of every class: N = 3 on every axis, N = 5 on one."""
    for kind in ("regular", "rectilinear"):
        for n, axes, per in ((3, (0, 1, 2), 2), (5, (3,), 1)):
            for axis in axes:
                case, cls = k1_probe_case(kind, PROBE_SHAPES[n], axis, np.float64)
                pick = np.concatenate([np.flatnonzero(cls == c)[:per] for c in range(5)])
                obs = [o[pick] for o in case.obs]
                kw = dict(starts=case.starts, steps=case.steps) if kind == "regular" else {}
                full = exact_rational.evaluate("cubic", kind, case.grids, case.vals, obs, linearize=False, **kw)
                along = _exact_along_axis(case, axis)
                assert [along[i][0] for i in pick] == full, (kind, n, axis)
