"""GPU parity tests of the BANDED SpMV plan (sprs_amd/csrc/spmv_band.hip: hot columns served from LDS,
16-bit local column ids, compact row lists per piece) against the CPU oracle — the same bar as
test_spmv_gpu.py: <= 1e-10 relative (north star), empty rows exact.  Reference semantics:
prod::mul_acc_mat_vec_csr, sprs/src/sparse/prod.rs:103-127.

The shapes below are chosen to hit the plan's corner cases at sizes the oracle handles in seconds:
rows spanning several hot tiles, ranges and workgroups (register and head carries), tiles full of row starts,
hot slices without entries, a cold rest in several label ranges, every index-width combination.

The SEAM CASES at the end reach the paths that exist only for edge shapes (more than 64 pieces, more than 64 head records in
a row block, tiles full of row ends, operands at odd doubles, infinite x beside padding, bucket and row-numbering limits) and
compare BIT FOR BIT: small-integer values and x make every summation order give the same double (check_band_exact)."""
import os

import numpy as np
import pytest

from conftest import IDX_COMBOS
from helpers import ragged_csr, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-10


@pytest.fixture(scope="module")
def hip():
    import sprs_amd
    if sprs_amd.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X (no CPU fallback exists)")
    return sprs_amd


class band_options:
    def __init__(self, hip, hot, phases, rounds=0, split=0, tile=0, cold_tiles=0, hot_run=0, overlap=0, tail=0):
        self.hip, self.vals = hip, dict(spmv_band=1, spmv_band_hot=hot, spmv_band_phases=phases, spmv_band_rounds=rounds,
                                        spmv_band_split=split, spmv_band_tile=tile, spmv_band_cold_tiles=cold_tiles,
                                        spmv_band_hot_run=hot_run, spmv_band_overlap=overlap, spmv_band_tail=tail)

    def __enter__(self):
        for k, v in self.vals.items():
            self.hip.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.vals:
            self.hip.set_option(k, 0)


def oracle_spmv(shape, ip, ix, dt, x, y=None):
    from oracle import oracle
    out = np.zeros(shape[0]) if y is None else y.copy()
    oracle.mul_acc_mat_vec_csr(shape, ip.astype(np.uint64), ix.astype(np.uint64), dt, x, out)   # same arithmetic at any width
    return out


def check_band(hip, shape, ip, ix, dt, seed=0, expect_kind=3):
    from sprs_amd import prod
    from sprs_amd.device import DeviceCsMat, DeviceVec
    rng = np.random.default_rng(seed)
    x = rng.random(shape[1]) + 0.5
    a = DeviceCsMat.from_host(shape, ip, ix, dt)
    xv = DeviceVec.from_host(x)
    y = (a * xv).to_host()
    assert a.spmv_plan_info()[0] == expect_kind
    ref = oracle_spmv(shape, ip, ix, dt, x)
    assert rel_err(y, ref) <= TOL
    empty = np.diff(ip.astype(np.int64)) == 0
    assert np.all(y[empty] == 0.0)
    # the repeat on the same handle takes ANOTHER x: a partial sum, a carry slot or an entry of the permuted x that the second
    # call fails to rewrite then holds the first call's value, not the right one
    xb = rng.random(shape[1]) + 0.5
    xbv = DeviceVec.from_host(xb)
    yb = (a * xbv).to_host()
    assert rel_err(yb, oracle_spmv(shape, ip, ix, dt, xb)) <= TOL
    assert np.all(yb[empty] == 0.0)
    assert np.array_equal(yb, (a * xbv).to_host())          # cached plan + scratch: bit-identical
    y0 = rng.random(shape[0]) + 0.5
    yv = DeviceVec.from_host(y0)
    prod.mul_acc_mat_vec_csr(a, xv, yv)                     # accumulate form (prod.rs:120-126), back on the first x
    y2 = yv.to_host()
    assert rel_err(y2, oracle_spmv(shape, ip, ix, dt, x, y=y0)) <= TOL
    assert np.array_equal(y2[empty], y0[empty])             # empty rows untouched, bit for bit
    return y


def check_band_exact(hip, shape, ip, ix, seed=0):
    """The plan against the oracle BIT FOR BIT: values and x are integers in 1 .. 4 (every product and every sum is an integer
    far below 2^53, so every order of the additions gives the same double — one stray, stale or missing addend changes the
    result), on ONE handle for three rounds with a fresh x each, operator and accumulate form in every round."""
    from sprs_amd import prod
    from sprs_amd.device import DeviceCsMat, DeviceVec
    rng = np.random.default_rng(seed)
    dt = rng.integers(1, 5, size=ix.size).astype(np.float64)
    lens = np.diff(ip.astype(np.int64))
    a = DeviceCsMat.from_host(shape, ip, ix, dt)

    def same(got, ref, what):
        bad = np.flatnonzero(got != ref)
        assert bad.size == 0, "%s: %d rows differ, first rows %s of lengths %s: got %s, oracle %s" % (
            what, bad.size, bad[:8].tolist(), lens[bad[:8]].tolist(), got[bad[:8]].tolist(), ref[bad[:8]].tolist())

    for rnd in range(3):
        x = rng.integers(1, 5, size=shape[1]).astype(np.float64)
        xv = DeviceVec.from_host(x)
        y = (a * xv).to_host()
        assert a.spmv_plan_info()[0] == 3                   # (a case that falls back to the plain tiles tests nothing)
        same(y, oracle_spmv(shape, ip, ix, dt, x), "round %d, y = A x" % rnd)
        y0 = rng.integers(1, 9, size=shape[0]).astype(np.float64)
        yv = DeviceVec.from_host(y0)
        prod.mul_acc_mat_vec_csr(a, xv, yv)
        assert a.spmv_plan_info()[0] == 3
        same(yv.to_host(), oracle_spmv(shape, ip, ix, dt, x, y=y0), "round %d, y += A x" % rnd)
    return a


def check_seam(hip, shape, ip, ix, dt, seed=0):
    """a seam case: the exact rounds, and one round of random doubles (the float path has its own roundings)"""
    check_band_exact(hip, shape, ip, ix, seed=seed)
    check_band(hip, shape, ip, ix, dt, seed=seed)


@pytest.mark.parametrize("idx,ptr", IDX_COMBOS + [(np.uint64, np.uint32)])
@pytest.mark.parametrize("hot,phases,tile", [(2, 1, 16384), (5, 3, 8192)])
def test_rmat_vs_oracle(hip, idx, ptr, hot, phases, tile):
    from sprs_amd import gen
    n = 50000
    indptr, indices, data = gen.rmat_csr(n, 16)
    ip, ix, dt = indptr.numpy().astype(ptr), indices.numpy().astype(idx), data.numpy()
    with band_options(hip, hot, phases, tile=tile):
        check_band(hip, (n, n), ip, ix, dt)


def test_hub_rows_and_many_segments(hip):
    """3 dense rows (20 000 entries each: every hot slice sees rows that span several tiles, ranges and workgroups ->
    register carries inside a range, head carries between ranges, runs of ranges without a row start) and 7 000 rows of
    33 entries (tiles in which every lane holds several row starts), short and empty rows in between; one to forty
    hot workgroups per CU, ranges of one tile up to a whole segment, one to seven tiles per cold range."""
    lens = [0, 20000, 3, 0] + [33] * 3500 + [20000] + [1, 0, 31, 32] * 50 + [33] * 3500 + [20000, 0, 0, 7]
    shape, ip, ix, dt = ragged_csr(lens, 20000, seed=3)
    for rounds, tile, ct, run in ((1, 8192, 4, 0), (3, 16384, 1, 1), (40, 8192, 7, 3), (2, 16384, 2, 1000)):
        with band_options(hip, 2, 2, rounds=rounds, tile=tile, cold_tiles=ct, hot_run=run):
            check_band(hip, shape, ip, ix, dt, seed=rounds)


def test_reduction_beside_the_short_rows(hip):
    """the two streams forced on a small matrix: the reduction of the long rows starts when the hot slices and the cold
    pieces are done and runs beside the short rows (whose carries follow them on the second stream) — the same additions in
    the same order as with the whole second stream joined first (spmv_band_tail = 2) and as on one stream: bit-identical"""
    from sprs_amd.device import DeviceCsMat, DeviceVec
    rng = np.random.default_rng(21)
    rows, cols = 6000, 300000
    lens = rng.integers(1, 60, size=rows)
    lens[::97] = 5000                                          # hub rows: runs that span ranges in the early slices
    lens[5::7] = 2500                                          # short rows (below the split) that span several cold tiles: carries into y
    lens[3::50] = 0
    shape, ip, ix, dt = ragged_csr(list(lens), cols, seed=22)
    x = rng.random(cols) + 0.5
    out = {}
    for overlap, tail in ((2, 0), (1, 0), (1, 2)):
        with band_options(hip, 12, 1, tile=8192, rounds=3, hot_run=2, split=3000, cold_tiles=1, overlap=overlap, tail=tail):
            check_band(hip, shape, ip, ix, dt, seed=4)
            a = DeviceCsMat.from_host(shape, ip, ix, dt)
            xv = DeviceVec.from_host(x)
            out[(overlap, tail)] = [(a * xv).to_host() for _ in range(3)]
    first = out[(2, 0)][0]
    for ys in out.values():
        for y in ys:
            assert np.array_equal(y, first)


def test_split_and_empty_pieces(hip):
    """all long rows live in a narrow column range: most hot slices and hash pieces have no entries; a second
    matrix has no short rows at all, a third no long rows (the banded plan does not apply: plain tiles)"""
    rng = np.random.default_rng(11)
    n, cols = 3000, 60000
    lens = rng.integers(40, 90, size=n)
    ip = np.zeros(n + 1, dtype=np.uint64)
    ip[1:] = np.cumsum(lens)
    ix = np.concatenate([np.sort(rng.choice(700, size=l, replace=False)) + 17000 for l in lens]).astype(np.uint64)
    dt = rng.random(ix.size) + 0.5
    with band_options(hip, 6, 2):
        check_band(hip, (n, cols), ip, ix, dt)
    with band_options(hip, 3, 1, split=2):
        shape, ip2, ix2, dt2 = ragged_csr([5, 9, 2, 64, 300] * 400, 30000, seed=5)
        check_band(hip, shape, ip2, ix2, dt2)
    with band_options(hip, 3, 1, split=1000):
        shape, ip3, ix3, dt3 = ragged_csr([5, 9, 0, 64, 300] * 100, 9000, seed=6)
        check_band(hip, shape, ip3, ix3, dt3, expect_kind=1)


def test_band_equals_sliced_and_plain_within_rounding(hip):
    """the three plans group the products of a row differently: equal to the oracle within tolerance, to each
    other within rounding"""
    from sprs_amd import gen
    from sprs_amd.device import DeviceCsMat, DeviceVec
    n = 40000
    indptr, indices, data = gen.rmat_csr(n, 24, seed=9)
    ip, ix, dt = indptr.numpy().astype(np.uint64), indices.numpy().astype(np.uint64), data.numpy()
    x = gen.dense_vector(n, seed=2).numpy()
    out = {}
    try:
        for name, opts in (("band", dict(spmv_band=1, spmv_band_hot=3)), ("sliced", dict(spmv_band=2, spmv_xcs=1)),
                           ("plain", dict(spmv_band=2, spmv_xcs=2))):
            for k, v in opts.items():
                hip.set_option(k, v)
            a = DeviceCsMat.from_host((n, n), ip, ix, dt)
            out[name] = (a * DeviceVec.from_host(x)).to_host()
            assert a.spmv_plan_info()[0] == {"band": 3, "sliced": 2, "plain": 1}[name]
    finally:
        for k in ("spmv_band", "spmv_band_hot", "spmv_xcs"):
            hip.set_option(k, 0)
    ref = oracle_spmv((n, n), ip, ix, dt, x)
    for name, y in out.items():
        assert rel_err(y, ref) <= TOL, name
    assert rel_err(out["band"], out["plain"]) <= 1e-13 and rel_err(out["band"], out["sliced"]) <= 1e-13


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_random_shapes_and_plan_options(hip, seed):
    """seeded random ragged matrices (empty rows, rows of one entry, rows around the split, hub rows, a column range nobody
    references) under random plan geometries — tile size, slices, phases, rounds, range lengths, cold range lengths, the
    two-part reduction — all against the oracle, the accumulate form and the bit-identical repeat included (check_band)"""
    rng = np.random.default_rng(1000 + seed)
    rows = int(rng.integers(200, 1500))
    cols = int(rng.integers(9000, 70000))
    kinds = rng.integers(0, 6, size=rows)
    lens = np.where(kinds == 0, 0, np.where(kinds == 1, 1, np.where(kinds == 2, rng.integers(20, 30, size=rows),
                    np.where(kinds == 3, rng.integers(2, 24, size=rows), rng.integers(24, 200, size=rows)))))
    hubs = rng.choice(rows, size=3, replace=False)
    lens[hubs] = rng.integers(2000, min(cols, 9000), size=3)
    shape, ip, ix, dt = ragged_csr([int(v) for v in lens], cols, seed=seed)
    ix = (ix.astype(np.int64) * 7 // 8).astype(ix.dtype)                 # the top eighth of the columns is never referenced ...
    for r in range(rows):                                                # ... (keep the rows strictly increasing)
        seg = ix[int(ip[r]):int(ip[r + 1])]
        if seg.size and np.any(np.diff(seg.astype(np.int64)) <= 0):
            ix[int(ip[r]):int(ip[r + 1])] = np.unique(seg)[:1].repeat(seg.size) + np.arange(seg.size, dtype=ix.dtype)
    ix = np.minimum(ix, cols - 1)
    ok = all(np.all(np.diff(ix[int(ip[r]):int(ip[r + 1])].astype(np.int64)) > 0) for r in range(rows))
    if not ok:
        pytest.skip("degenerate draw")
    tile = int(rng.choice([8192, 16384]))
    hot = int(rng.integers(1, max(2, cols // tile + 1)))
    opts = dict(rounds=int(rng.integers(1, 6)), tile=tile, cold_tiles=int(rng.integers(1, 6)), hot_run=int(rng.integers(1, 6)),
                split=int(rng.choice([2, 8, 24, 40])))
    with band_options(hip, hot, int(rng.integers(1, 4)), **opts):
        check_band(hip, shape, ip, ix, dt, seed=seed)


@pytest.mark.skipif(bool(os.environ.get("SPRS_HIP_LIBRARY")), reason="torch streams: real device only")   # (the emulator run)
@pytest.mark.parametrize("kind,opts", [(3, dict(spmv_band=1)), (2, dict(spmv_band=2, spmv_xcs=1))], ids=["banded", "sliced"])
def test_plan_built_on_a_nonblocking_stream(hip, kind, opts):
    """a plan prepared on a torch stream (hipStreamNonBlocking: not ordered with the null stream) and multiplied there at once
    is the plan the null stream builds — its read-backs wait for the kernels of that stream: same kind, same bytes, same bits.
    The banded plan of this R-MAT lays its short rows out in buckets (split 8, one wave tile per cold tile)"""
    import torch
    from sprs_amd import gen, prod
    from sprs_amd.device import DeviceCsMat, DeviceVec
    n = 200000
    indptr, indices, data = gen.rmat_csr(n, 16, seed=5)
    ip, ix, dt = indptr.numpy().astype(np.uint64), indices.numpy().astype(np.uint64), data.numpy()
    assert (np.diff(ip.astype(np.int64)) < 8).any()                    # short rows: the bucketed short piece is in use
    x = DeviceVec.from_host(gen.dense_vector(n, seed=6).numpy())
    s = torch.cuda.Stream(device=torch.device("cuda", 0))
    out = []
    try:
        for k, v in opts.items():
            hip.set_option(k, v)
        for stream in (s, None):
            a = DeviceCsMat.from_host((n, n), ip, ix, dt).prepare(stream=stream)
            y = DeviceVec.from_host(np.zeros(n))
            prod.mul_acc_mat_vec_csr(a, x, y, stream=stream)            # no host synchronise since prepare
            if stream is not None:
                stream.synchronize()
            out.append((a.spmv_plan_info(), y.to_host()))
    finally:
        for k in opts:
            hip.set_option(k, 0)
    (info_s, y_s), (info_0, y_0) = out
    assert info_s[0] == kind and info_s == info_0
    assert np.array_equal(y_s, y_0)


# ---------------------------------------------------------------------------------------------
# SEAM CASES: the smallest shapes that reach the paths of the plan which exist only for edge shapes, each checked bit for bit
# (check_band_exact) and once with random doubles (check_band).  Every case asserts that the banded plan was taken.
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cold_tiles", [1, 4])
def test_short_tiles_full_of_row_ends(hip, cold_tiles):
    """short tiles with more than 256 and with exactly 512 row ends (rows of one entry): the rows whose place in y was not
    requested ahead (emit_y, m >= 4) and all four staging windows of band_tile_sums, in ranges of one and of four tiles"""
    lens = [600] * 3 + [1] * 2500 + [2, 1, 1, 0, 3] * 200 + [1] * 700 + [600]
    shape, ip, ix, dt = ragged_csr(lens, 30000, seed=1)
    with band_options(hip, 2, 1, tile=8192, split=8, cold_tiles=cold_tiles):
        check_seam(hip, shape, ip, ix, dt, seed=1)


def test_hot_tiles_full_of_row_ends(hip):
    """every row is long (split 2): hot tiles with more row ends than a staging window holds (nf > STG), the last window
    parked until the next tile's loads are requested"""
    lens = [2, 3, 2, 4] * 1500 + [700]
    shape, ip, ix, dt = ragged_csr(lens, 40000, seed=2)
    with band_options(hip, 4, 1, tile=8192, split=2, hot_run=3):
        check_seam(hip, shape, ip, ix, dt, seed=2)


def test_more_than_64_head_records_in_a_row_block(hip):
    """100 long rows (fewer than 128: natural order) of ~1300 entries per slice in single-tile ranges: the first block of 64
    long rows owns about two records of heads per row, so the reduction reloads its record lanes (i0 != sb)"""
    lens = [3, 0] * 20 + [2600] * 100 + [5] * 30
    shape, ip, ix, dt = ragged_csr(lens, 16384, seed=3)
    with band_options(hip, 2, 1, tile=8192, split=8, hot_run=1, rounds=1):
        check_seam(hip, shape, ip, ix, dt, seed=3)


def test_hub_run_of_many_ranges(hip):
    """two hub rows that run through far more than 8 single-tile ranges of a slice: their heads are cut into records of eight
    carries, added by the h_n loop of the reduction"""
    lens = [9, 0, 3] * 10 + [16000] + [40] * 64 + [12000, 2]
    shape, ip, ix, dt = ragged_csr(lens, 16384, seed=12)
    with band_options(hip, 2, 1, tile=8192, split=8, hot_run=1, rounds=1):
        check_seam(hip, shape, ip, ix, dt, seed=12)


def test_more_than_64_pieces(hip):
    """60 hot slices + 8 cold pieces = 68 pieces, table rows of 80: the second chunk of 64 table rows in the reduction and the
    k += 64 loops of the plan build.  Eight rows reference EVERY column between them, so the labels reach all 60 slices and
    the cold rest (with random rows alone the labels in use end long before the last slice)"""
    cols = 61 * 8192 - 100
    cover = [np.arange(r, cols, 8) for r in range(8)]
    rest = [3000] * 70 + [4] * 100 + [0, 9] * 30
    _, _, ix2, dt2 = ragged_csr(rest, cols, seed=4)
    lens = [c.size for c in cover] + rest
    ip = np.zeros(len(lens) + 1, dtype=np.uint64)
    ip[1:] = np.cumsum(lens)
    ix = np.concatenate(cover + [ix2.astype(np.int64)]).astype(np.uint64)
    dt = np.concatenate([np.random.default_rng(4).random(cols) + 0.5, dt2])
    assert np.unique(ix).size == cols
    with band_options(hip, 60, 1, tile=8192, split=8):
        check_seam(hip, (len(lens), cols), ip, ix, dt, seed=4)


@pytest.mark.parametrize("cols,form", [(9001, "scatter"), (30001, "gather")])
def test_operands_at_odd_doubles(hip, cols, form):
    """the ABI takes raw device pointers: x and / or y at an address that is 8 mod 16 (one double into a longer buffer) take the
    scalar branches of band_permute_kernel (most columns referenced) and of band_gather_kernel (a third or fewer referenced),
    for the copy of x and for the clearing of y — empty rows at every residue mod 4 and at the very end, rows and columns no
    multiple of 4.  The doubles in front of and behind y stay as they were."""
    import ctypes as C
    from sprs_amd import _ffi
    from sprs_amd.device import DeviceCsMat, DeviceVec
    rng = np.random.default_rng(5)
    lens = [700, 3, 0, 5, 0, 0, 0, 0, 2] * 30 + [1] * (2 if form == "scatter" else 3) + [0] * 5
    (rows, _), ip, ix, dtr = ragged_csr(lens, 9000, seed=5)          # columns below 9 000
    shape = (rows, cols)
    assert rows % 4 and cols % 4 and ((np.unique(ix).size * 3 <= cols) == (form == "gather"))
    empty = np.flatnonzero(np.diff(ip.astype(np.int64)) == 0)
    assert set((empty % 4).tolist()) == {0, 1, 2, 3} and empty[-1] == rows - 1
    dt = rng.integers(1, 5, size=ix.size).astype(np.float64)
    with band_options(hip, 1, 1, tile=8192, split=8):
        check_seam(hip, shape, ip, ix, dtr, seed=5)
        a = DeviceCsMat.from_host(shape, ip, ix, dt)
        for xo, yo in ((1, 0), (0, 1), (1, 1)):
            for acc in (0, 1):
                x = rng.integers(1, 5, size=cols).astype(np.float64)
                y0 = rng.integers(1, 5, size=rows).astype(np.float64)
                xb = DeviceVec.from_host(np.concatenate([[77.0] * xo, x, [77.0]]))
                yb = DeviceVec.from_host(np.concatenate([[55.0] * yo, y0, [55.0]]))
                assert (xb.ptr + 8 * xo) % 16 == 8 * xo and (yb.ptr + 8 * yo) % 16 == 8 * yo
                _ffi.check(_ffi.lib.sprs_hip_spmv_f64(a._h, C.c_void_p(xb.ptr + 8 * xo), cols, C.c_void_p(yb.ptr + 8 * yo), rows, acc, None))
                assert a.spmv_plan_info()[0] == 3
                got = yb.to_host()
                ref = oracle_spmv(shape, ip, ix, dt, x, y=y0 if acc else None)
                bad = np.flatnonzero(got[yo:yo + rows] != ref)
                assert bad.size == 0, (xo, yo, acc, bad[:8].tolist(), got[yo:yo + rows][bad[:8]].tolist(), ref[bad[:8]].tolist())
                assert got[-1] == 55.0 and got[0] == (55.0 if yo else ref[0])      # the neighbours of y


def test_infinite_x_and_padding(hip):
    """the padding behind a piece's last entry (hot: value 0, id 0 = the slice's first label) must not turn an infinite x into a NaN
    in another row.  Even rows use even columns, odd rows odd ones; x is +inf on one group's columns, then on the other's —
    whichever column got a slice's first label is infinite in one of the two runs — and the rows of the finite group must
    come out as the oracle's finite values (the whole vector is compared, infinities included)."""
    from sprs_amd.device import DeviceCsMat, DeviceVec
    rng = np.random.default_rng(6)
    cols = 40000
    lens = [900, 37, 5, 0, 12, 300] * 40
    (rows, _), ip, ix, dtr = ragged_csr(lens, cols // 2, seed=6)
    ix = 2 * ix + np.repeat(np.arange(rows, dtype=np.uint64) & 1, np.diff(ip.astype(np.int64)))
    shape = (rows, cols)
    dt = rng.integers(1, 5, size=ix.size).astype(np.float64)
    with band_options(hip, 3, 2, tile=8192, split=8, hot_run=1):
        check_seam(hip, shape, ip, ix, dtr, seed=6)
        a = DeviceCsMat.from_host(shape, ip, ix, dt)
        for group in (0, 1):
            x = rng.integers(1, 5, size=cols).astype(np.float64)
            x[group::2] = np.inf
            y = (a * DeviceVec.from_host(x)).to_host()
            assert a.spmv_plan_info()[0] == 3
            ref = oracle_spmv(shape, ip, ix, dt, x)
            assert np.isfinite(ref[(np.arange(rows) & 1) != group]).all() and not np.isnan(ref).any()
            bad = np.flatnonzero(~((y == ref) | (np.isnan(y) & np.isnan(ref))))
            assert np.array_equal(y, ref, equal_nan=True), (group, bad[:8].tolist(), y[bad[:8]].tolist(), ref[bad[:8]].tolist())


@pytest.mark.parametrize("lens", [[5] * 201 + [3, 5] + [900] * 2, [7] * 72 + [1] + [7] * 72 + [900]], ids=["last_bucket_empty", "row_ends_at_505"])
def test_bucket_seams_of_the_short_piece(hip, lens):
    """split 8 and single-tile ranges: buckets of R' = 512 - 7 = 505 entries.  A row that starts exactly at 505 and a last row
    that straddles 1010, which leaves the last bucket empty (bp_bucket_starts_kernel, nnz_short_padded); a row of one entry
    that ends exactly at 505 (short_place)"""
    shape, ip, ix, dt = ragged_csr(lens, 20000, seed=7)
    with band_options(hip, 1, 1, tile=8192, split=8, cold_tiles=1):
        check_seam(hip, shape, ip, ix, dt, seed=7)


@pytest.mark.parametrize("n_long", [63, 64, 65, 127, 128, 129, 61 * 64 - 1, 61 * 64, 61 * 64 + 1, 62 * 64 + 5])
def test_long_row_numbering(hip, n_long):
    """long_row_number deals the first B = min(n_long / 64, 61) blocks' rows round-robin: B < 2 (natural order), B = every full
    block, the cap at 61 with rows behind it — and the last, partial block of the reduction"""
    lens = [3, 0] + [8, 9] * (n_long // 2) + [8] * (n_long % 2) + [0, 2]
    shape, ip, ix, dt = ragged_csr(lens, 12000, seed=n_long)
    assert (np.asarray(lens) >= 8).sum() == n_long
    with band_options(hip, 1, 1, tile=8192, split=8):
        check_seam(hip, shape, ip, ix, dt, seed=n_long)


def test_split_boundary_and_tiny_shares(hip):
    """rows of split - 1, split and split + 1 entries (bp_classify_kernel), rows that end exactly at a tile, and hot workgroups
    of one, two and five tiles: segments that start in the middle of a slice and of a row"""
    lens = [7, 8, 9, 0, 1] * 300 + [1024, 512, 511, 513] + [8] * 64
    shape, ip, ix, dt = ragged_csr(lens, 17000, seed=9)
    for share in (1, 2, 5):
        try:
            hip.set_option("spmv_band_share", share)
            with band_options(hip, 2, 1, tile=8192, split=8, hot_run=1):
                check_seam(hip, shape, ip, ix, dt, seed=share)
        finally:
            hip.set_option("spmv_band_share", 0)
