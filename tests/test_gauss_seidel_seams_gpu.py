"""Seam cases of the device Gauss-Seidel sweep (sprs_amd/csrc/gauss_seidel.hip): the systolic band schedule behind option
gauss_seidel_chain = S (gs_band_kernel, gs_band_check_kernel, the per-handle cache of the check in gs_impl) away from the 5-point
Laplacian it was written around, and the launch options of the level-order sweep (gauss_seidel_xcd / _blocks / _naps).

Everything is compared with oracle.gauss_seidel, the restatement of the reference's sweep (sprs/examples/heat.rs:103-139): every
iterate BIT FOR BIT (np.array_equal on the doubles; where the oracle holds a NaN: also a NaN), the sweep counts, and the
convergence scalar by same_error of tests/test_gauss_seidel_gpu.py (1e-10 of sum |r_i|).  No other tolerance.

The schedule is restated here from first principles (band_place): a band is 64 S consecutive rows, lane = (i - B) // S owns the
chain of S rows, t = (i - B) % S is the row's place in it, and the row is swept at step lane + t.  A stored c < i may be read iff
it lies in an earlier band or is swept at an earlier step; where the kernel finds its value depends on which of those it is:
  prev            c == i - 1, t > 0                 the lane's own previous row: the LDS ring
  above           c == i - S, lane > 0              what the lane above swept a step ago: the LDS ring
  inband_polled   any other B <= c < i              fetched 16 steps ahead (always still pending), polled at the use
  earlier_band    c < B                             waited for two turns ahead of the use (lane 0's row above; any lane here)
  later           c > i                             the previous iterate
Each test asserts that the kinds it exists for occur in its input.
(tests/test_emu_cpu.py runs this file through the CPU emulator of the kernels under three wave orders.)"""
import contextlib
import functools

import numpy as np
import pytest

from conftest import IDX_COMBOS
from test_gauss_seidel_gpu import EMU, _random_system, heat_system, same_error

pytestmark = pytest.mark.gpu

ALL_ONES = np.frombuffer(np.uint64(0xFFFFFFFFFFFFFFFF).tobytes(), dtype=np.float64)[0]
KINDS = ("prev", "above", "inband_polled", "earlier_band", "earlier_band_lane_gt0", "later")


@pytest.fixture(scope="module")
def hip():
    import sprs_amd
    if sprs_amd.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X (no CPU fallback exists)")
    return sprs_amd


@contextlib.contextmanager
def options(hip, **opts):
    """options off their defaults for the length of a block; put back in a finally"""
    defaults = {name: hip.get_option(name) for name in opts}
    try:
        for name, value in opts.items():
            hip.set_option(name, value)
        yield defaults
    finally:
        for name, value in defaults.items():
            hip.set_option(name, value)


# ---------------------------------------------------------------------------------------------------------------------------------
# the schedule, restated
# ---------------------------------------------------------------------------------------------------------------------------------
def band_place(i, S):
    """(B, lane, t) of row i under stride S"""
    B = i // (64 * S) * (64 * S)
    return B, (i - B) // S, (i - B) % S


def band_step(i, S):
    _, lane, t = band_place(i, S)
    return lane + t


def band_allows(c, i, S):
    """may row i store column c under stride S"""
    if c > i:
        return True
    B, _, _ = band_place(i, S)
    return c < B or band_step(c, S) < band_step(i, S)


def band_kind(c, i, S):
    """the operand source of a stored column c != i of row i (a tuple: an earlier-band column of a lane > 0 counts twice)"""
    B, lane, t = band_place(i, S)
    if c > i:
        return ("later",)
    if c < B:
        return ("earlier_band", "earlier_band_lane_gt0") if lane > 0 else ("earlier_band",)
    if c == i - 1 and t > 0:
        return ("prev",)
    if c == i - S and lane > 0:
        return ("above",)
    return ("inband_polled",)


class System:
    """a sorted CSR system (int64 arrays; arrays() casts), its right-hand side and start vector, and what its entries exercise"""

    def __init__(self, n, ip, ix, dt, rhs, x0, key=None):
        self.n, self.ip, self.ix, self.dt, self.rhs, self.x0, self.key = n, ip, ix, dt, rhs, x0, key

    def arrays(self, idx=np.uint64, ptr=np.uint64):
        return (self.n, self.n), self.ip.astype(ptr), self.ix.astype(idx), self.dt

    def row(self, i):
        return [int(c) for c in self.ix[self.ip[i]:self.ip[i + 1]]]

    def counts(self, S):
        out = dict.fromkeys(KINDS + ("rows8", "rows1", "diag_places"), 0)
        places = set()
        for i in range(self.n):
            cols = self.row(i)
            places.add(cols.index(i))
            out["rows8"] += len(cols) == 8
            out["rows1"] += len(cols) == 1
            for c in cols:
                if c != i:
                    for k in band_kind(c, i, S):
                        out[k] += 1
        out["diag_places"] = len(places)                        # at how many places of a row the diagonal is found
        return out

    def fits(self, S):
        """what gs_band_check_kernel decides, restated"""
        return all(len(self.row(i)) <= 8 and all(band_allows(c, i, S) for c in self.row(i) if c != i) for i in range(self.n))

    def with_entries(self, i, cols, value=0.25):
        """a copy with columns `cols` added to row i (kept sorted; the diagonal's margin of 1 + u outweighs four such entries)"""
        old = self.row(i)
        assert not set(cols) & set(old) and all(0 <= c < self.n for c in cols)
        new = sorted(old + list(cols))
        vals = dict(zip(old, self.dt[self.ip[i]:self.ip[i + 1]]))
        vals.update({c: value for c in cols})
        lo, hi = int(self.ip[i]), int(self.ip[i + 1])
        ix = np.concatenate([self.ix[:lo], np.array(new, dtype=np.int64), self.ix[hi:]])
        dt = np.concatenate([self.dt[:lo], np.array([vals[c] for c in new]), self.dt[hi:]])
        ip = self.ip.copy()
        ip[i + 1:] += len(cols)
        return System(self.n, ip, ix, dt, self.rhs, self.x0)


@functools.lru_cache(maxsize=None)
def band_fit_system(n, S, seed):
    """a random system that fits the band schedule of stride S: per row 0, 1, 3, 5, 7 or 7 off-diagonal columns drawn from the
    columns around the row's band neighbours, the band edge, the ends of the matrix and four random ones, filtered by
    band_allows; off-diagonals standard normal x 10^k, k in -3 .. 3; a dominant diagonal of either sign, so the iterates stay
    finite; rhs and x0 standard normal.  Returns (System, counts by operand source + rows of 8 and of 1 entries + places of the
    diagonal); built once per (n, S, seed) — the index and pointer widths are chosen where the handle is made (Solver)."""
    rng = np.random.default_rng(seed)
    ip, ix, dt = [0], [], []
    for i in range(n):
        B, _, _ = band_place(i, S)
        cand = [i - 1, i - 2, i - 3, i - S, i - S - 1, i - S + 1, i - 2 * S, i - 2 * S - 1, B - 1, B - S, 0,
                i + 1, i + 2, i + S, i + S - 1, n - 1] + [int(c) for c in rng.integers(0, n, size=4)]
        ok = []
        for c in cand:
            if 0 <= c < n and c != i and c not in ok and band_allows(c, i, S):
                ok.append(c)
        k = (0, 1, 3, 5, 7, 7)[int(rng.integers(6))]
        cols = [ok[j] for j in rng.permutation(len(ok))[:k]]
        off = {c: rng.standard_normal() * 10.0 ** int(rng.integers(-3, 4)) for c in cols}
        diag = (sum(abs(v) for v in off.values()) + 1.0 + rng.random()) * (1.0 if rng.random() < 0.5 else -1.0)
        off[i] = diag
        for c in sorted(off):
            ix.append(c)
            dt.append(off[c])
        ip.append(len(ix))
    s = System(n, np.array(ip, dtype=np.int64), np.array(ix, dtype=np.int64), np.array(dt), rng.standard_normal(n), rng.standard_normal(n),
               key=(n, S, seed))
    return s, s.counts(S)


_REFS = {}


def reference(s, max_iter, eps):
    """(x_ref, info, sum |r_i|) of the oracle's sweep — computed once per (system, sweeps, eps), handed out read-only"""
    from oracle import oracle
    import scipy.sparse as sp
    key = (s.key, max_iter, eps)
    if s.key is None or key not in _REFS:
        shape, ip, ix, dt = s.arrays()
        x_ref, info = oracle.gauss_seidel(shape, ip, ix, dt, s.x0, s.rhs, max_iter, eps)
        with np.errstate(invalid="ignore", over="ignore"):
            scale = np.abs(sp.csr_matrix((s.dt, s.ix, s.ip), shape=shape) @ x_ref - s.rhs).sum()
        x_ref.setflags(write=False)
        if s.key is None:
            return x_ref, info, scale
        _REFS[key] = (x_ref, info, scale)
    return _REFS[key]


class Solver:
    """ONE DeviceCsMat handle for any number of solves: the level order and the band check's verdict are kept on it"""

    def __init__(self, s, idx=np.uint64, ptr=np.uint64):
        from sprs_amd.device import DeviceCsMat
        self.s = s
        self.a = DeviceCsMat.from_host(*s.arrays(idx, ptr))

    def solve(self, max_iter, eps, stream=None):
        from sprs_amd.device import DeviceVec
        from sprs_amd.linalg import gauss_seidel
        x = DeviceVec.from_host(self.s.x0)
        res = gauss_seidel(self.a, x, DeviceVec.from_host(self.s.rhs), max_iter, eps, stream=stream)
        return x.to_host(), res

    def check(self, max_iter, eps, stream=None):
        """a solve under the options in force against the oracle: bits and counts; the error scalar where the sweeps are counted
        out (eps < 0), like tests/test_gauss_seidel_gpu.py.  In a run TO convergence the r_i are what the rounding of the residual
        SpMV leaves of them, and the device's SpMV adds a row in another order than the oracle's: sum r_i then differs in its leading
        digits (n = 1161, S = 9, sweep 127: 1.7104e-07 against 1.6476e-07 with sum |r_i| = 1.5e-11; n = 1000, S = 999, sweep 198:
        9.6340e-07 against 9.6328e-07; device and emulator alike) although the iterates are the same bits — nothing that
        same_error's 1e-10 of sum |r_i| is about.  DESIGN.md 4.5."""
        x_ref, info, scale = reference(self.s, max_iter, eps)
        x, res = self.solve(max_iter, eps, stream)
        print("n = %d, max_iter %d, eps %g: iterations %d / %d, error %r / %r" % (self.s.n, max_iter, eps, res.iterations, info["iterations"],
                                                                                res.error, info["error"]))
        assert np.array_equal(x, x_ref)
        assert (res.iterations, res.converged) == (info["iterations"], bool(info["converged"]))
        if eps < 0:
            assert same_error(res.error, info["error"], scale)
        return res


def refused(hip, s, S, idx=np.uint64, ptr=np.uint64):
    with options(hip, gauss_seidel_chain=S):
        with pytest.raises(hip.SprsHipError) as e:
            Solver(s, idx, ptr).solve(1, -1.0)
    assert e.value.status == hip._ffi.INVALID_ARG
    return True


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. systems that fit a band schedule, at the strides and sizes where the kernel's bookkeeping changes
# ---------------------------------------------------------------------------------------------------------------------------------
# (n, S): the generator's seed; the number of bands; n % S != 0 (a chain that ends early); the last band holds fewer than 64 chains;
# in-band polls can exist; a band after the first has a lane > 0 (the wait for an earlier band's row from another lane than 0)
BAND_CASES = {
    (3, 2): dict(seed=207, bands=1, ragged=True, short_band=True, polled=False, gt0=False),     # smallest stride, the full 3 x 3
    (131, 2): dict(seed=201, bands=2, ragged=True, short_band=True, polled=True, gt0=True),
    (193, 3): dict(seed=301, bands=2, ragged=True, short_band=True, polled=True, gt0=False),    # (its second band is ONE row)
    (64 * 7 * 2 + 5 * 7 + 3, 7): dict(seed=701, bands=3, ragged=True, short_band=True, polled=True, gt0=True),   # S around GB_WAVES = 8:
    (64 * 8 + 1, 8): dict(seed=801, bands=2, ragged=True, short_band=True, polled=True, gt0=False),              # a chain is shorter than
    (64 * 9 * 2 + 9, 9): dict(seed=901, bands=3, ragged=False, short_band=True, polled=True, gt0=True),          # the prefetch distance
    (64 * 64 + 64 * 3 + 5, 64): dict(seed=6401, bands=2, ragged=True, short_band=True, polled=True, gt0=True),
    (65 * 64 * 2 - 1, 65): dict(seed=6501, bands=2, ragged=True, short_band=False, polled=True, gt0=True),       # a chain longer than the lanes are many
    (1000, 999): dict(seed=99901, bands=1, ragged=True, short_band=True, polled=True, gt0=False),   # the largest stride: one chain and one row
}


def band_case(n, S):
    return band_fit_system(n, S, BAND_CASES[(n, S)]["seed"])


@pytest.mark.parametrize("idx,ptr", IDX_COMBOS)
@pytest.mark.parametrize("n,S", list(BAND_CASES))
def test_band_fit_systems_bit_for_bit(hip, n, S, idx, ptr):
    """one and three sweeps, and the sweeps to convergence (eps 1e-6, at most 200), of band_fit_system(n, S) under
    gauss_seidel_chain = S, at every index / pointer width; then the level-order kernel on the SAME handle: the same bits"""
    if EMU and n > 1200:
        pytest.skip("emulator: small systems only")
    if EMU and S == 999 and idx is not np.uint64:
        pytest.skip("emulator: 1062 steps of eight polling waves take 9 s; the 32-bit widths are emulated at the other strides")
    s, counts = band_case(n, S)
    facts = BAND_CASES[(n, S)]
    band = 64 * S
    last = (n - 1) // band * band
    print(n, S, counts)
    # the case must hold what it is here for
    assert -(-n // band) == facts["bands"]
    assert (n % S != 0) == facts["ragged"]
    assert (-(-(n - last) // S) < 64) == facts["short_band"]
    assert (facts["bands"] >= 3 or (last > 0 and n - last > S)) == facts["gt0"]        # some band after the first has a second chain
    assert (counts["inband_polled"] > 0) == facts["polled"]
    assert (counts["earlier_band"] > 0) == (facts["bands"] >= 2)
    assert (counts["earlier_band_lane_gt0"] > 0) == facts["gt0"]
    assert counts["prev"] > 0 and counts["above"] > 0 and counts["later"] > 0
    assert (counts["rows8"] > 0 and counts["rows1"] > 0 and counts["diag_places"] >= 7) == (n > 3)      # (all 8 at most shapes)
    assert s.fits(S)
    solver = Solver(s, idx, ptr)
    runs = [(1, -1.0), (3, -1.0), (200, 1e-6)]
    with options(hip, gauss_seidel_chain=S):
        for max_iter, eps in runs:
            solver.check(max_iter, eps)
    assert hip.get_option("gauss_seidel_chain") == 0
    for max_iter, eps in runs:                                  # level order, same handle
        solver.check(max_iter, eps)


@pytest.mark.skipif(EMU, reason="more bands than CUs: real device only (the emulator runs one workgroup after the other: there every "
                                "case of several bands draws them all with one workgroup)")
def test_band_redraws_bands(hip):
    """more bands than workgroups launched (one per CU at most): a workgroup draws a second band — step_done is armed again, the
    LDS ring still holds the rows of the band before"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    S = 2
    n = 128 * (cus + 3) + 5
    assert n > 128 * cus, "one band per workgroup: nothing is redrawn"
    s, counts = band_fit_system(n, S, 7)
    assert counts["inband_polled"] > 0 and counts["earlier_band_lane_gt0"] > 0 and counts["prev"] > 0 and counts["above"] > 0
    with options(hip, gauss_seidel_chain=S):
        Solver(s).check(2, -1.0)


@pytest.mark.skipif(EMU, reason="a torch stream: real device only")
def test_band_on_a_nonblocking_stream(hip):
    """the band sweep and its check kernel on a torch stream (hipStreamNonBlocking: not ordered with the null stream)"""
    import torch
    stream = torch.cuda.Stream(device=torch.device("cuda", 0))
    s, counts = band_case(193, 3)
    assert counts["inband_polled"] > 0
    with options(hip, gauss_seidel_chain=3):
        Solver(s).check(3, -1.0, stream=stream.cuda_stream)           # (a fresh handle: the check kernel runs on the stream too)
        Solver(s).check(3, -1.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. NaN of all-ones payload and a zero diagonal, read through every operand source
# ---------------------------------------------------------------------------------------------------------------------------------
def _special_system():
    """S = 4, n = 64 * 4 + 7, by hand.  Every row holds its diagonal and i + 1; the chains' first rows (t = 0) also i - 4, their
    second rows (t = 1) also i - 1.  Row R = 41 (lane 10, t = 1) is read by R + 1 (prev), R + 4 (above), R + 2 and R + 5 (in-band,
    polled), by rows 257 (lane 0) and 261 (lane 1) of the second band (earlier band) and by row R - 1 (later: the previous
    iterate) — and none of these readers stores another row that depends on R in the same sweep: what row R publishes reaches
    each of them through ONE source"""
    S, n, R = 4, 64 * 4 + 7, 41
    rows = []
    for i in range(n):
        _, lane, t = band_place(i, S)
        cols = {i: 4.0}
        if i + 1 < n:
            cols[i + 1] = -0.5
        if t == 0 and i - S >= 0:
            cols[i - S] = 0.75
        if t == 1:
            cols[i - 1] = -1.0
        rows.append(cols)
    for i, v in ((R + 1, 0.875), (R + S, -0.25), (R + 2, 0.375), (R + S + 1, -0.625), (257, 1.5), (261, -0.125)):
        assert R not in rows[i]
        rows[i][R] = v
    ip = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    ix = np.array([c for r in rows for c in sorted(r)], dtype=np.int64)
    dt = np.array([r[c] for r in rows for c in sorted(r)])
    rng = np.random.default_rng(41)
    return System(n, ip, ix, dt, rng.standard_normal(n), rng.standard_normal(n)), S, R


@pytest.mark.parametrize("case", ["nan_all_ones_in_rhs", "stored_zero_diagonal"])
def test_band_special_values(hip, case):
    """(a) rhs[R] is the NaN whose bits are the band kernel's 'not swept yet' word: published as another NaN, it must reach the
    rows that read row R out of the LDS ring, by the poll at the use and by the wait for an earlier band as a VALUE — none of them
    may wait for it for ever ('never published').  (b) a stored 0.0 on the diagonal of row R: inf / NaN iterates like the
    reference, through the same paths.  NaN where the oracle has one, the oracle's bits everywhere else."""
    from oracle import oracle
    s, S, R = _special_system()
    assert s.fits(S)
    readers = {k: [i for i in range(s.n) if R in s.row(i) and i != R and k in band_kind(R, i, S)] for k in KINDS}
    assert readers["prev"] == [R + 1] and readers["above"] == [R + S] and readers["inband_polled"] == [R + 2, R + S + 1]
    assert readers["earlier_band"] == [257, 261] and readers["earlier_band_lane_gt0"] == [261] and readers["later"] == [R - 1]
    if case == "nan_all_ones_in_rhs":
        s.rhs[R] = ALL_ONES
        assert s.rhs[R:R + 1].view(np.uint64)[0] == 0xFFFFFFFFFFFFFFFF
    else:
        (p,) = [p for p in range(int(s.ip[R]), int(s.ip[R + 1])) if s.ix[p] == R]
        s.dt[p] = 0.0
    shape, ip, ix, dt = s.arrays()
    for sweeps in (1, 2):
        with np.errstate(all="ignore"):
            x_ref, info = oracle.gauss_seidel(shape, ip, ix, dt, s.x0, s.rhs, sweeps, 1e-9)
        bad = set(np.flatnonzero(~np.isfinite(x_ref)).tolist())
        if sweeps == 1:                                          # row R and its six readers of this sweep, nothing else
            assert bad == {R, R + 1, R + 2, R + S, R + S + 1, 257, 261}
        else:
            assert bad > {R - 1, R, R + 1, R + 2, R + S, R + S + 1, 257, 261} and len(bad) < s.n
        with options(hip, gauss_seidel_chain=S):
            x, res = Solver(s).solve(sweeps, 1e-9)
        assert np.array_equal(np.isnan(x), np.isnan(x_ref))
        ok = ~np.isnan(x_ref)
        assert np.array_equal(x[ok], x_ref[ok])
        assert not res.converged and info["converged"] == 0 and res.iterations == sweeps


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the check kernel from both sides of its two conditions, and the cache of its verdict
# ---------------------------------------------------------------------------------------------------------------------------------
def _find_row(s, S, want, room=1):
    """the first row that satisfies want(i, B, lane, t) and has room for `room` more entries"""
    for i in range(s.n):
        if len(s.row(i)) + room <= 8 and want(i, *band_place(i, S)):
            return i
    raise AssertionError("no such row")


def _free_later(s, i, k):
    """k columns behind row i that it does not store yet (always allowed)"""
    cols = [c for c in range(i + 1, s.n) if c not in s.row(i)][:k]
    assert len(cols) == k
    return cols


def _free_earlier_band(s, i, S, k):
    B, _, _ = band_place(i, S)
    cols = [c for c in range(B) if c not in s.row(i)][:k]
    assert len(cols) == k
    return cols


@pytest.mark.parametrize("n,S", [(193, 3), (64 * 7 * 2 + 38, 7)])
def test_band_check_both_sides(hip, n, S):
    """single-entry mutations of a fitting system on both sides of gs_band_check_kernel's two conditions (rows of at most 8
    entries; every stored c < i of the row's band swept at an earlier step): what the restated schedule allows is solved, bit for
    bit; what it does not allow is refused with INVALID_ARG — in the first row, the last row and the last, partial band"""
    s, _ = band_case(n, S)
    assert s.fits(S) and n % 256 != 0
    band = 64 * S
    last = (n - 1) // band * band
    accepted, rejected = {}, {}

    # -- rows of exactly 8 and of 9 entries
    i = _find_row(s, S, lambda i, B, lane, t: i > 0 and 2 <= len(s.row(i)) < 8 and i + 9 < n)
    accepted["8 entries"] = s.with_entries(i, _free_later(s, i, 8 - len(s.row(i))))
    assert len(accepted["8 entries"].row(i)) == 8
    rejected["9 entries, row 0"] = s.with_entries(0, _free_later(s, 0, 9 - len(s.row(0))))
    rejected["9 entries, row n - 1"] = s.with_entries(n - 1, _free_earlier_band(s, n - 1, S, 9 - len(s.row(n - 1))))
    i = last if n - last == 1 else last + 1
    if i != n - 1:
        assert last > 0 and last < i < n - 1
        rejected["9 entries, last band"] = s.with_entries(i, _free_earlier_band(s, i, S, 9 - len(s.row(i))))
    else:
        assert (n, S) == (193, 3)                               # (its last band IS row n - 1)
    for name, m in rejected.items():
        assert max(len(m.row(r)) for r in range(n)) == 9 and all(band_allows(c, r, S) for r in range(n) for c in m.row(r) if c != r), name

    # -- the column right of the row above: from the chain's last row that is the chain's own FIRST row (S - 1 steps early, polled);
    #    from the row before it, the last row of the chain above: the same step
    i = _find_row(s, S, lambda i, B, lane, t: lane > 0 and t == S - 1 and i - S + 1 not in s.row(i))
    accepted["i - S + 1 at t = S - 1"] = s.with_entries(i, [i - S + 1])
    assert band_step(i - S + 1, S) == band_step(i, S) - (S - 1) and band_kind(i - S + 1, i, S) == ("inband_polled",)
    i = _find_row(s, S, lambda i, B, lane, t: lane > 0 and t == S - 2 and i - S + 1 not in s.row(i))
    rejected["i - S + 1 at t = S - 2"] = s.with_entries(i, [i - S + 1])
    assert band_step(i - S + 1, S) == band_step(i, S)

    # -- the row before a chain's first row: the earlier band for lane 0, the END of the chain above for every other lane
    i = _find_row(s, S, lambda i, B, lane, t: B > 0 and lane == 0 and t == 0 and i - 1 not in s.row(i))
    accepted["i - 1 at t = 0, lane 0, second band"] = s.with_entries(i, [i - 1])
    assert band_kind(i - 1, i, S)[0] == "earlier_band"
    i = _find_row(s, S, lambda i, B, lane, t: lane > 0 and t == 0 and i - 1 not in s.row(i))
    rejected["i - 1 at t = 0, lane > 0"] = s.with_entries(i, [i - 1])
    assert band_step(i - 1, S) == band_step(i, S) + S - 2

    # -- the column left of the row above: two steps early, polled at the use
    i = _find_row(s, S, lambda i, B, lane, t: lane > 0 and t > 0 and i - S - 1 not in s.row(i))
    accepted["i - S - 1 at t > 0"] = s.with_entries(i, [i - S - 1])
    assert band_kind(i - S - 1, i, S) == ("inband_polled",) and band_step(i - S - 1, S) == band_step(i, S) - 2

    # -- a violation in the very last row (the check's last, partial workgroup)
    B, _, _ = band_place(n - 1, S)
    late = [c for c in range(B, n - 1) if not band_allows(c, n - 1, S) and c not in s.row(n - 1)]
    if late:
        rejected["a violation in row n - 1"] = s.with_entries(n - 1, late[:1])
    else:
        assert (n, S) == (193, 3) and B == n - 1                # (every column before its last row lies in an earlier band)

    assert len(accepted) == 4 and len(rejected) == {193: 4, 934: 6}[n]
    for name, m in accepted.items():
        assert m.fits(S), name
        with options(hip, gauss_seidel_chain=S):
            Solver(m).check(2, -1.0)
    for name, m in rejected.items():
        assert not m.fits(S), name
        for idx, ptr in IDX_COMBOS:                              # (the check kernel at every index / pointer width)
            assert refused(hip, m, S, idx, ptr), name
        Solver(m).check(1, -1.0)                               # (nothing wrong with the system: level order sweeps it)

    # -- the stride against the number of rows
    for bad_S in (n, n + 5):
        assert refused(hip, s, bad_S)
    wide, _ = band_fit_system(n, n - 1, 5)                           # S = n - 1: one chain of n - 1 rows, and lane 1 with the last row
    assert wide.fits(n - 1) and not s.fits(n - 1)
    with options(hip, gauss_seidel_chain=n - 1):
        Solver(wide).check(2, -1.0)
    assert refused(hip, s, n - 1)
    with options(hip, gauss_seidel_chain=1):                   # 1 is no stride: level order, not an error
        Solver(s).check(2, -1.0)


def test_band_cache_follows_the_stride(hip):
    """gs_impl keeps the check's verdict on the handle, keyed by the stride: one handle under a stride that fits, one that does
    not (twice: the second refusal comes from the cache), the first again, and level order; a second handle with another
    structure is judged on its own"""
    S1, S2 = 3, 5
    s, _ = band_case(193, S1)
    assert s.fits(S1) and not s.fits(S2)
    solver = Solver(s)
    with options(hip, gauss_seidel_chain=S1):
        solver.check(2, -1.0)
    for _ in range(2):
        with options(hip, gauss_seidel_chain=S2):
            with pytest.raises(hip.SprsHipError) as e:
                solver.solve(2, -1.0)
        assert e.value.status == hip._ffi.INVALID_ARG
    with options(hip, gauss_seidel_chain=S1):
        solver.check(2, -1.0)
    solver.check(2, -1.0)
    i = _find_row(s, S1, lambda i, B, lane, t: lane > 0 and t == 0 and i - 1 not in s.row(i))
    other = s.with_entries(i, [i - 1])
    assert not other.fits(S1)
    with options(hip, gauss_seidel_chain=S1):
        second = Solver(other)
        with pytest.raises(hip.SprsHipError) as e:
            second.solve(2, -1.0)
        assert e.value.status == hip._ffi.INVALID_ARG
        solver.check(3, -1.0)                                  # the first handle's verdict is untouched
    second.check(2, -1.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the launch options of the level-order sweep
# ---------------------------------------------------------------------------------------------------------------------------------
def levels_of(s):
    """level(i) = 1 + max level(c) over the stored c < i; the number of levels"""
    lv = np.zeros(s.n, dtype=np.int64)
    for i in range(s.n):
        below = [c for c in s.row(i) if c < i]
        lv[i] = 1 + max(lv[c] for c in below) if below else 0
    return int(lv.max()) + 1


@functools.lru_cache(maxsize=None)
def _launch_systems():
    import scipy.sparse as sp
    out = []
    rows = 24 if EMU else 96
    shape, ip, ix, dt, rhs = heat_system(rows)
    out.append(System(shape[0], ip.astype(np.int64), ix.astype(np.int64), dt, rhs, np.random.default_rng(3).standard_normal(shape[0]), key="heat"))
    n = 500 if EMU else 3000
    a = _random_system(n, 11 + n, 6, 400)
    rng = np.random.default_rng(n)
    rhs, x0 = rng.standard_normal(n), rng.standard_normal(n)
    out.append(System(n, a.indptr.astype(np.int64), a.indices.astype(np.int64), a.data, rhs, x0, key="random"))
    n = 200 if EMU else 1000
    a = (sp.diags(np.full(n, 2.0)) + sp.diags(np.full(n - 1, -1.0), -1)).tocsr()
    out.append(System(n, a.indptr.astype(np.int64), a.indices.astype(np.int64), a.data, np.arange(1, n + 1, dtype=np.float64), np.zeros(n), key="chain"))
    return [(s, levels_of(s)) for s in out]


@pytest.mark.parametrize("opts", [{"gauss_seidel_xcd": 1}, {"gauss_seidel_blocks": 1}, {"gauss_seidel_blocks": 3},
                                  {"gauss_seidel_blocks": 65536}, {"gauss_seidel_naps": 64},
                                  {"gauss_seidel_xcd": 1, "gauss_seidel_blocks": 1}],
                         ids=lambda o: "-".join("%s=%d" % (k[13:], v) for k, v in o.items()))
def test_sweep_launch_options_bit_for_bit(hip, opts):
    """the options that pick the instantiation (ONE_XCD: only the workgroups that find themselves on XCD 0 sweep), the grid and the
    back-off of gs_sweep_kernel, one off its default at a time (and the one-XCD sweep with a single workgroup's worth of grid):
    three sweeps of the heat system, of a random non-symmetric system with a row of hundreds of entries and of the bidiagonal
    chain give the oracle's bits, level count, sweep count and error"""
    systems = _launch_systems()
    assert systems[0][1] == 2 * (24 if EMU else 96) - 4 and systems[2][1] == systems[2][0].n
    for name, value in opts.items():
        assert value != hip.get_option(name), name
    with options(hip, **opts):
        assert hip.get_option("gauss_seidel_chain") == 0
        for s, levels in systems:
            res = Solver(s).check(3, -1.0)
            assert res.levels == levels
