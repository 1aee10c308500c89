"""What the library puts on the caller's stream around its kernels, and what must still hold without it.

A launch through a scratch block (sweep, sorted and slice paths) used to be followed by two event records, one for the block
and one for the stream, and `finish()` by an 8-byte copy.  Now a launch is followed by nothing: a block remembers the stream
that used it last and its event is recorded only when ANOTHER stream takes the block (or the block is freed), closing a handle
waits for the streams it was given, and `finish()` brings the status word — a field set's K words together — to the host with
ONE one-lane kernel (option `finish_kernel`, default 1) in front of the runtime's wait for the stream.  The tests below are the cases in which
that laziness could show: a block handed between streams, reuse on one stream, an event recorded before `finish()`, a handle
closed with work in flight, the K status words of a field set behind one command, and a stream under capture (which must not
be touched at all).

Every result is compared BIT FOR BIT with the oracle.  Every test runs under a watchdog of its own: a call that never comes
back ends the process with a traceback instead of waiting.
"""

import faulthandler

import numpy as np
import pytest

from tests.helpers import run_oracle, synthetic_case

pytestmark = pytest.mark.gpu

KNOBS = ("BRICKS", "SWEEP", "SWEEP_PROBE", "SWEEP_PERIOD", "BINNED", "COLUMN", "FINISH_KERNEL", "FORCE_GENERIC", "BIN_SLICE_LOG2")
UNREP = "Unrepresentable coordinate value"


@pytest.fixture(autouse=True)
def _watchdog():
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for name in KNOBS:
        monkeypatch.delenv("INTERPN_HIP_" + name, raising=False)


def _same_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64, what
    same = (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), (what, int((~same).sum()), np.argwhere(~same)[:4].ravel().tolist())


def _open(which, interpn_amd, monkeypatch):
    """One of the two paths that work in a scratch block of the handle, forced at a size where a test takes a moment: the
    sweep kernel (3-D multilinear, 9 x 8 x 7, 20 000 points) or the counting sort in front of the tiled multicubic kernel
    (4-D, 6^4, 5 000 points).  Returns (case, handle, the path's name, the counter that must move)."""
    if which == "sweep":
        case = synthetic_case("linear", "regular", 3, [9, 8, 7], 20_000, 4101, np.float64, extrap=0.2)
        monkeypatch.setenv("INTERPN_HIP_BRICKS", "11")  # (a grid this small keeps no re-laid table, and so no sweep table, by itself)
        it = interpn_amd.Interpolator.regular("linear", case.dims, case.starts, case.steps, case.vals)
        monkeypatch.delenv("INTERPN_HIP_BRICKS")
        it.set_option("sweep", 1)
        assert it.get_option("sweep_table_bytes") > 0
        return case, it, "sweep", "evals_sweep"
    case = synthetic_case("cubic", "regular", 4, [6, 6, 6, 6], 5_000, 4102, np.float64, extrap=0.2, specials=False)
    monkeypatch.setenv("INTERPN_HIP_BRICKS", "11")
    it = interpn_amd.Interpolator.regular("cubic", case.dims, case.starts, case.steps, case.vals)
    monkeypatch.delenv("INTERPN_HIP_BRICKS")
    it.set_option("binned", 1)
    it.set_option("column", 0)
    return case, it, "binned", "evals_binned"


@pytest.mark.parametrize("which", ["sweep", "sorted"])
def test_block_handed_between_streams(oracle, monkeypatch, which):
    """Launches alternate between two streams with no `finish` in between.  The handle has ONE scratch block (allocation is
    forbidden after the first launch has made it), so every launch takes the block the other stream used last: the one case
    in which the block's event is recorded late, on the other stream, by the stream that now wants the block.  Without that
    event two launches would work in the block at once.

    The status word is one per handle, so what `finish(stream)` reports is the smallest failing index of whatever has run by
    then: with the failing point of the stream finished FIRST in front of the other stream's, its index is what that call must
    report, and the other call reports its own stream's index or nothing (the first call has reset the word: it depends on
    whether the other stream's launches had finished by then)."""
    import torch

    import interpn_amd

    dev = torch.device("cuda:0")
    case, it, path, counter = _open(which, interpn_amd, monkeypatch)
    n = case.obs[0].size
    want = run_oracle(oracle, case, True)
    try:
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        bad_at = [n // 3 + 11, n // 2 + 7]  # stream 0's failing point lies in front of stream 1's
        obs = []
        for k in range(2):
            cols = [torch.from_numpy(o).to(dev) for o in case.obs]
            cols[k][bad_at[k]] = float("nan")
            cols[2][n - 5 - k] = float("inf")  # a later failure must not win
            obs.append(cols)
        outs = [torch.zeros(n, dtype=torch.float64, device=dev) for _ in range(8)]
        torch.cuda.synchronize()
        for k in range(8):
            with torch.cuda.stream(streams[k % 2]):
                it.eval_tensors(obs[k % 2], outs[k], no_alloc=k > 0)
            assert it.last_path == path, (k, it.last_path, it.last_path_reason)
        assert it.get_option("scratch_allocs") == 1 and it.get_option(counter) == 8
        with pytest.raises(AssertionError, match=UNREP) as err:
            it.finish(streams[0])
        assert err.value.first_bad_index == bad_at[0]
        try:
            it.finish(streams[1])
        except AssertionError as late:
            assert UNREP in str(late) and late.first_bad_index == bad_at[1]
        for k in range(8):
            good = np.ones(n, dtype=bool)
            good[[bad_at[k % 2], n - 5 - k % 2]] = False
            _same_bits(outs[k].cpu().numpy()[good], want[good], (which, k))
        # the other order: the stream finished first is the one whose failing point comes second in the arrays -> swap them
        for k in range(4):
            with torch.cuda.stream(streams[k % 2]):
                it.eval_tensors(obs[1 - k % 2], outs[k], no_alloc=True)
        with pytest.raises(AssertionError, match=UNREP) as err:
            it.finish(streams[1])
        assert err.value.first_bad_index == bad_at[0]
        try:
            it.finish(streams[0])
        except AssertionError as late:
            assert late.first_bad_index == bad_at[1]
        assert it.get_option("scratch_allocs") == 1
    finally:
        it.close()


@pytest.mark.parametrize("which", ["sweep", "sorted"])
def test_fifty_launches_on_one_stream(oracle, monkeypatch, which):
    """Reuse of a block by the stream that used it last needs no event at all: 50 launches on one stream, one `finish`, every
    result the oracle's bits, every launch on the forced path, one block."""
    import torch

    import interpn_amd

    dev = torch.device("cuda:0")
    case, it, path, counter = _open(which, interpn_amd, monkeypatch)
    n = case.obs[0].size
    want = run_oracle(oracle, case, True)
    try:
        side = torch.cuda.Stream()
        obs = [torch.from_numpy(o).to(dev) for o in case.obs]
        outs = torch.zeros((50, n), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for k in range(50):
                it.eval_tensors(obs, outs[k])
                assert it.last_path == path
        it.finish()
        got = outs.cpu().numpy()
        for k in range(50):
            _same_bits(got[k], want, (which, k))
        assert it.get_option(counter) == 50 and it.get_option("evals_in_place") == 0
        assert it.get_option("scratch_allocs") == 1
    finally:
        it.close()


@pytest.mark.parametrize("finish_kernel", [0, 1])
def test_event_recorded_before_finish_is_complete(oracle, finish_kernel):
    """An event recorded between the launch and `finish()` reads complete when `finish()` returns, 2 000 times out of 2 000,
    with the status word delivered by the copy (0) or by the one-lane kernel (1, the default).  `finish()` ends in the runtime's
    wait for the stream: while it watched the landing word instead, the host could see the word before the runtime had retired
    the event in front of it (64, 85 and 116 of 2 000 events late in three runs with the copy)."""
    import torch

    import interpn_amd

    dev = torch.device("cuda:0")
    case = synthetic_case("linear", "regular", 3, [9, 8, 7], 4096, 4103, np.float64, extrap=0.2)
    want = run_oracle(oracle, case, True)
    it = interpn_amd.Interpolator.regular("linear", case.dims, case.starts, case.steps, case.vals)
    try:
        assert it.get_option("finish_kernel") == 1  # the default
        it.set_option("finish_kernel", finish_kernel)
        obs = [torch.from_numpy(o).to(dev) for o in case.obs]
        out = torch.zeros(4096, dtype=torch.float64, device=dev)
        events = [torch.cuda.Event() for _ in range(8)]
        late = 0
        for k in range(2000):
            it.eval_tensors(obs, out)
            ev = events[k % 8]
            ev.record()
            it.finish()
            late += not ev.query()
        assert late == 0, (finish_kernel, late)
        _same_bits(out.cpu().numpy(), want)
    finally:
        it.close()


@pytest.mark.parametrize("which", ["sweep", "sorted"])
def test_close_with_work_in_flight(oracle, monkeypatch, which):
    """Closing a handle waits for the streams it was given (nothing was recorded on them at launch time) before its blocks go
    back to the pool: five launches on a side stream, no `finish`, close; a second handle then takes those blocks from the
    pool, and both handles' results are the oracle's."""
    import torch

    import interpn_amd

    dev = torch.device("cuda:0")
    case, it, path, counter = _open(which, interpn_amd, monkeypatch)
    n = case.obs[0].size
    want = run_oracle(oracle, case, True)
    side = torch.cuda.Stream()
    obs = [torch.from_numpy(o).to(dev) for o in case.obs]
    outs = torch.zeros((5, n), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(side):
            for k in range(5):
                it.eval_tensors(obs, outs[k])
                assert it.last_path == path
    finally:
        it.close()
    assert side.query()  # close has waited for the stream
    case2, it2, path2, _ = _open(which, interpn_amd, monkeypatch)
    try:
        got2 = it2.eval_tensors(obs)
        assert it2.last_path == path2
        it2.finish()
        _same_bits(got2.cpu().numpy(), want, which)
    finally:
        it2.close()
    got = outs.cpu().numpy()
    for k in range(5):
        _same_bits(got[k], want, (which, k))


@pytest.mark.parametrize("fused", [0, 1])
def test_field_set_finish(oracle, fused):
    """K = 3 fields: on the per-field path (`fused` = 0) every field's handle has a status word of its own, and `finish()`
    brings all three to the host behind one command (the default, and `finish_kernel` = 1); the fused kernel reports through
    the first handle's word alone.  A batch with a failing point raises the same text with the same `.first_bad_index` either
    way — and with the words delivered by copies, handle by handle (`finish_kernel` = 0), as before — and leaves the words
    clean for the batch without one."""
    import torch

    import interpn_amd

    dev = torch.device("cuda:0")
    K, n, bad_at = 3, 10_000, 6_321
    case = synthetic_case("linear", "regular", 3, [5, 6, 7], n, 4104, np.float64, extrap=0.2, specials=False)
    rng = np.random.default_rng(4105)
    vals = rng.uniform(-1.0, 1.0, (K, case.vals.size))
    want = np.zeros((K, n))
    for f in range(K):
        oracle.linear_regular(case.dims, case.starts, case.steps, vals[f], case.obs, want[f])
    fs = interpn_amd.Fields.regular("linear", case.dims, case.starts, case.steps, vals)
    try:
        fs.set_option("fused", fused)
        clean = [torch.from_numpy(o).to(dev) for o in case.obs]
        bad = [c.clone() for c in clean]
        bad[1][bad_at] = float("nan")
        bad[0][bad_at + 1000] = float("inf")
        good = np.ones(n, dtype=bool)
        good[[bad_at, bad_at + 1000]] = False
        for finish_kernel in (1, 0, 1):
            fs.set_option("finish_kernel", finish_kernel)
            got = fs.eval_tensors(bad)
            assert fs.last_path == ("fused" if fused else "per_field")
            with pytest.raises(AssertionError) as err:
                fs.finish()
            assert str(err.value) == UNREP and err.value.first_bad_index == bad_at, (finish_kernel, str(err.value))
            _same_bits(got.cpu().numpy()[:, good], want[:, good], (fused, finish_kernel))
            got = fs.eval_tensors(clean)
            fs.finish()
            _same_bits(got.cpu().numpy(), want, (fused, finish_kernel))
    finally:
        fs.close()


@pytest.mark.parametrize("which", ["sweep", "sorted"])
def test_capture_is_not_touched(oracle, monkeypatch, which):
    """A launch on a stream under capture (one stream, no parallel branches) still says "stream under graph capture", runs the
    one-pass kernel, records nothing, and the replayed graph gives the oracle's bits; the block an earlier launch left behind
    on ANOTHER stream is not asked about while that goes on."""
    import torch

    import interpn_amd

    dev = torch.device("cuda:0")
    case, it, path, counter = _open(which, interpn_amd, monkeypatch)
    n = case.obs[0].size
    want = run_oracle(oracle, case, True)
    try:
        obs = [torch.from_numpy(o).to(dev) for o in case.obs]
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            first = it.eval_tensors(obs)  # leaves a block behind whose last use is on `side`
        assert it.last_path == path
        it.finish()
        res = torch.zeros(n, dtype=torch.float64, device=dev)
        before = it.get_option(counter)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            it.eval_tensors(obs, res)
        assert it.last_path == "in_place" and "capture" in it.last_path_reason, (it.last_path, it.last_path_reason)
        assert it.get_option(counter) == before
        assert float(res.abs().max()) == 0.0  # captured, not run
        graph.replay()
        torch.cuda.synchronize()
        _same_bits(res.cpu().numpy(), want, which)
        _same_bits(first.cpu().numpy(), want, which)
        again = it.eval_tensors(obs)  # and the handle goes on as before
        assert it.last_path == path
        it.finish()
        _same_bits(again.cpu().numpy(), want, which)
        del graph
    finally:
        it.close()


# ---------------------------------------------------------------------------------------------------------------------
# The previous use REALLY still in flight.  In the cases above a kernel of a few microseconds has long finished when the
# other stream takes its block (the host side of a call is ~45 us), so they would pass without the wait in take_bin_slot or
# the stream waits in interpn_hip_destroy.  Here a device-side delay of at least 0.5 s sits in front of the library's launch,
# and the host looks 50 ms later: a 10x margin, a condition of the test and not a measurement.

STALL_S = 0.5
LOOK_S = 0.05
_cycles_per_s = []


def _stall(torch):
    """Enqueues a delay on the current stream and returns the pair of events around it; `_stalled_long_enough` asserts
    afterwards that it lasted STALL_S.  The cycle count is calibrated once, with two events."""
    if not _cycles_per_s:
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1_000_000)  # (first launch of the kernel: not timed)
        torch.cuda.synchronize()
        t0.record()
        torch.cuda._sleep(20_000_000)
        t1.record()
        t1.synchronize()
        _cycles_per_s.append(20_000_000 / (t0.elapsed_time(t1) * 1e-3))
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    torch.cuda._sleep(int(1.5 * STALL_S * _cycles_per_s[0]))
    t1.record()
    return t0, t1


def _stalled_long_enough(pair):
    pair[1].synchronize()
    assert pair[0].elapsed_time(pair[1]) >= STALL_S * 1e3, pair[0].elapsed_time(pair[1])


@pytest.mark.parametrize("which", ["sweep", "sorted"])
def test_other_stream_waits_for_a_stalled_use(oracle, monkeypatch, which):
    """ONE block.  Stream A is stalled and then launches into the block; stream B launches with allocation forbidden, so it
    gets A's block and must wait for A's use on the device: 50 ms later B's event is not complete (A is still stalled), the
    launch took the forced path, and there is still one block.  The control, same stall: a launch on B through a SECOND
    handle (its own block) in front of that has its event complete by then — the runtime does run the two streams side by
    side, so the pending event is the library's wait and nothing else.  Afterwards every result has the oracle's bits."""
    import time

    import torch

    import interpn_amd

    dev = torch.device("cuda:0")
    case, it, path, counter = _open(which, interpn_amd, monkeypatch)
    _, other, _, _ = _open(which, interpn_amd, monkeypatch)
    n = case.obs[0].size
    want = run_oracle(oracle, case, True)
    try:
        a, b = torch.cuda.Stream(), torch.cuda.Stream()
        obs = [torch.from_numpy(o).to(dev) for o in case.obs]
        outs = torch.zeros((4, n), dtype=torch.float64, device=dev)
        with torch.cuda.stream(a):
            it.eval_tensors(obs, outs[0])  # makes the one block
        with torch.cuda.stream(b):
            other.eval_tensors(obs, outs[1])  # ... and the second handle's
        torch.cuda.synchronize()
        outs.zero_()
        torch.cuda.synchronize()
        e_control, e_b = torch.cuda.Event(), torch.cuda.Event()
        with torch.cuda.stream(a):
            stall = _stall(torch)
            it.eval_tensors(obs, outs[0], no_alloc=True)
            assert it.last_path == path
        with torch.cuda.stream(b):
            other.eval_tensors(obs, outs[1], no_alloc=True)
            assert other.last_path == path
            e_control.record()
            it.eval_tensors(obs, outs[2], no_alloc=True)
            taken = (it.last_path, it.last_path_reason)
            e_b.record()
        time.sleep(LOOK_S)
        control_done, b_done, a_done = e_control.query(), e_b.query(), stall[1].query()
        allocs = it.get_option("scratch_allocs")
        a.synchronize()
        b.synchronize()
        _stalled_long_enough(stall)
        assert not a_done  # the stall was still on when the host looked
        assert control_done, "the runtime serialised the two streams: the next assertion would show nothing"
        assert not b_done, "stream B did not wait for the stalled use of the block it was handed"
        assert taken[0] == path, taken
        assert allocs == 1 and it.get_option(counter) == 3
        got = outs.cpu().numpy()
        for k in range(3):
            _same_bits(got[k], want, (which, k))
    finally:
        it.close()
        other.close()


@pytest.mark.parametrize("which", ["sweep", "sorted"])
def test_close_waits_for_a_stalled_stream(oracle, monkeypatch, which):
    """A stalled side stream, three launches, an event, `close()`: when `close()` returns the event is complete (it has waited
    at least the stall out), a second handle that takes the blocks from the pool gives the oracle's bits, and so do the three
    results."""
    import torch

    import interpn_amd

    dev = torch.device("cuda:0")
    case, it, path, counter = _open(which, interpn_amd, monkeypatch)
    n = case.obs[0].size
    want = run_oracle(oracle, case, True)
    side = torch.cuda.Stream()
    obs = [torch.from_numpy(o).to(dev) for o in case.obs]
    outs = torch.zeros((3, n), dtype=torch.float64, device=dev)
    ev = torch.cuda.Event()
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(side):
            stall = _stall(torch)
            for k in range(3):
                it.eval_tensors(obs, outs[k])
                assert it.last_path == path
            ev.record()
        assert not ev.query()  # (the stall is on)
    finally:
        it.close()
    assert ev.query(), "close() returned with the handle's work still in flight"
    _stalled_long_enough(stall)
    _, it2, path2, _ = _open(which, interpn_amd, monkeypatch)
    try:
        got2 = it2.eval_tensors(obs)
        assert it2.last_path == path2
        it2.finish()
        _same_bits(got2.cpu().numpy(), want, which)
    finally:
        it2.close()
    got = outs.cpu().numpy()
    for k in range(3):
        _same_bits(got[k], want, (which, k))


def test_reserve_regrows_only_after_the_stalled_use(oracle, monkeypatch):
    """The sorted path's block grows with the batch.  A stalled stream, a 5 000-point launch, an event; `reserve(50_000, 1)`
    must regrow the block — free it and allocate a larger one — and may do so only once the launch has run: on return there
    are two allocations and the event is complete.  The result has the oracle's bits."""
    import torch

    import interpn_amd

    dev = torch.device("cuda:0")
    case, it, path, counter = _open("sorted", interpn_amd, monkeypatch)
    n = case.obs[0].size
    want = run_oracle(oracle, case, True)
    try:
        side = torch.cuda.Stream()
        obs = [torch.from_numpy(o).to(dev) for o in case.obs]
        out = torch.zeros(n, dtype=torch.float64, device=dev)
        ev = torch.cuda.Event()
        with torch.cuda.stream(side):
            it.eval_tensors(obs, out)  # makes the block
        torch.cuda.synchronize()
        out.zero_()
        torch.cuda.synchronize()
        assert it.get_option("scratch_allocs") == 1
        with torch.cuda.stream(side):
            stall = _stall(torch)
            it.eval_tensors(obs, out, no_alloc=True)
            assert it.last_path == path
            ev.record()
        assert not ev.query()  # (the stall is on)
        it.reserve(50_000, 1)
        done = ev.query()
        assert it.get_option("scratch_allocs") == 2
        assert done, "reserve freed the block with its last use still in flight"
        _stalled_long_enough(stall)
        it.finish()
        _same_bits(out.cpu().numpy(), want)
    finally:
        it.close()
