"""SEAM CASES of the nnz-tile and XCD-sliced SpMV plans and of the one-wave-per-row kernel (sprs_amd/csrc/spmv.hip with
spmv_shared.hpp), BIT FOR BIT.  Reference semantics: prod::mul_acc_mat_vec_csr, sprs/src/sparse/prod.rs:103-127.

Values are integers in 1 .. 4 and x is a permutation of 1 .. cols: every product and every partial sum is an integer far below
2^53 (asserted per case), so EVERY order of the additions gives the same double, and one missing, stale, doubled or mislabelled
addend changes the result.  The reference is the product in int64 (prefix sums over the entries, differenced at indptr: no
floating-point order at all); the oracle must equal it too.  check_exact runs three rounds on one handle with a fresh x each,
operator and accumulate form in every round; the accumulate form starts every second empty row at -0.0 (the reference leaves
y untouched there, and -0.0 + 0.0 is +0.0), compared by its 8 bytes.  Every multiply asserts the plan kind it ran on
(1 plain tiles, 2 XCD-sliced, 0 none: the row-wave kernel), every case starts on fresh (poisoned) blocks, and every case adds one
round of random doubles against the oracle at the 1e-10 of test_spmv_gpu.py.

Constants of the kernels as the cases assume them: T = spmv_tile (2048 or 4096), SEG_CHUNK = 2048 row starts staged per pass,
LONG_SEG = 64 (segments from there on are summed by a wave), BLOCK = 256, 8 slices, RL_CHUNK = 1024 columns per wave of the
relabelling.  spmv_band = 2 keeps the banded plan out of every case."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers
from conftest import IDX_COMBOS
from helpers import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-10
EMU = bool(os.environ.get("SPRS_HIP_LIBRARY"))                       # (the kernel emulator of tests/emu)
device_only = pytest.mark.skipif(EMU, reason="launch-grid sizes and torch streams: real device only")
U32, U64 = np.uint32, np.uint64
W2 = [(U64, U64), (U32, U32)]
W4 = IDX_COMBOS + [(U64, U32)]
TILES = [2048, 4096]
SPMV_DEFAULTS = dict(spmv_kernel=0, spmv_xcs=0, spmv_xcs_split=32, spmv_xcs_idx32=1, spmv_tile=0, spmv_sort_tiles=0,
                     spmv_relabel=0, spmv_band=0)                     # common.hpp


@pytest.fixture(scope="module")
def hip():
    import sprs_amd
    if sprs_amd.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X (no CPU fallback exists)")
    return sprs_amd


class spmv_options:
    """the SpMV options of a case, every one of them back at its default afterwards (the `finally` of the case)"""

    def __init__(self, hip, **vals):
        assert set(vals) <= set(SPMV_DEFAULTS)
        self.hip, self.vals = hip, dict(vals, spmv_band=2)

    def __enter__(self):
        for k, v in self.vals.items():
            self.hip.set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in SPMV_DEFAULTS.items():
            self.hip.set_option(k, v)


def wname(idx, ptr):
    return "%s-%s" % (np.dtype(idx).name, np.dtype(ptr).name)


def seam_csr(lens, cols=None, seed=0, idx=U64, ptr=U64, pins=()):
    """structure with the given row lengths, built without a loop over the rows: ascending distinct column ids (a start and a
    stride drawn per row); `pins` gives the ids of chosen rows, (row, ids)"""
    lens = np.asarray(lens, dtype=np.int64)
    if cols is None:
        cols = int(lens.max(initial=0)) + 37
    assert lens.max(initial=0) <= cols
    rng = np.random.default_rng(seed)
    n = lens.size
    ip = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=ip[1:])
    row = np.repeat(np.arange(n), lens)
    pos = np.arange(ip[-1]) - ip[row]
    base = rng.integers(0, cols - lens + 1)
    gap = rng.integers(1, np.maximum(1, (cols - 1 - base) // np.maximum(lens - 1, 1)) + 1)
    ix = base[row] + pos * gap[row]
    for r, ids in pins:
        ids = np.asarray(ids, dtype=np.int64)
        assert ids.size == lens[r] and np.all(np.diff(ids) > 0) and ids[-1] < cols
        ix[ip[r]:ip[r + 1]] = ids
    assert ix.size == 0 or (ix.min() >= 0 and ix.max() < cols)
    return (n, cols), ip.astype(ptr), ix.astype(idx)


def int64_spmv(ip, ix, dt, x):
    """A x in int64: prefix sums over the entries, differenced at the row bounds — no floating-point order enters"""
    p = ip.astype(np.int64)
    cs = np.zeros(ix.size + 1, dtype=np.int64)
    np.cumsum(dt.astype(np.int64) * x.astype(np.int64)[ix.astype(np.int64)], out=cs[1:])
    return cs[p[1:]] - cs[p[:-1]]


def oracle_spmv(shape, ip, ix, dt, x, y=None):
    from oracle import oracle
    out = np.zeros(shape[0]) if y is None else y.copy()
    oracle.mul_acc_mat_vec_csr(shape, ip.astype(U64), ix.astype(U64), dt, x, out)   # same arithmetic at any width
    return out


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(U64)


class Exact:
    """one handle with integer values; round() multiplies it by a fresh permutation of 1 .. cols in both forms and compares
    every row with the int64 product"""

    def __init__(self, hip, shape, ip, ix, tile, seed=0):
        from sprs_amd.device import DeviceCsMat
        helpers.fresh_blocks()                       # results and scratch land in poisoned blocks: a word nobody wrote is seen
        self.shape, self.ip, self.ix, self.tile = shape, ip, ix, tile
        self.rng = np.random.default_rng(seed)
        self.dt = self.rng.integers(1, 5, size=ix.size).astype(np.float64)
        self.lens = np.diff(ip.astype(np.int64))
        self.empty = self.lens == 0
        self.a = DeviceCsMat.from_host(shape, ip, ix, self.dt)
        self.rounds = 0

    def same(self, got, ref, what):
        bad = np.flatnonzero(~(got == ref))
        first = bad[:8]
        assert bad.size == 0, "%s: %d rows differ, first rows %s of lengths %s, their first entries in tiles %s: got %s, expected %s" % (
            what, bad.size, first.tolist(), self.lens[first].tolist(), (self.ip.astype(np.int64)[first] // self.tile).tolist(),
            got[first].tolist(), ref[first].tolist())
        e = np.flatnonzero(self.empty)
        badz = e[bits(got)[e] != bits(ref)[e]]
        assert badz.size == 0, "%s: %d empty rows differ in their bytes, first rows %s: got %s, expected %s" % (
            what, badz.size, badz[:8].tolist(), got[badz[:8]].tolist(), ref[badz[:8]].tolist())

    def round(self, kind, stream=None):
        from sprs_amd import prod
        from sprs_amd.device import DeviceVec
        rows, cols = self.shape
        tag = "round %d" % self.rounds
        self.rounds += 1
        x = (self.rng.permutation(cols) + 1).astype(np.float64)
        exact = int64_spmv(self.ip, self.ix, self.dt, x)
        # all addends are positive: the largest row sum bounds every partial sum of every order, and below 2^53 all are exact
        assert exact.max(initial=0) + 8 < 2 ** 53
        ref = exact.astype(np.float64)
        assert np.array_equal(bits(oracle_spmv(self.shape, self.ip, self.ix, self.dt, x)), bits(ref)), tag + ": oracle, y = A x"
        xv = DeviceVec.from_host(x)
        yv = prod.csmat_mul_vec(self.a, xv, stream=stream)
        if stream is not None:
            stream.synchronize()
        assert self.a.spmv_plan_info()[0] == kind          # (a case that silently runs another plan tests nothing)
        self.same(yv.to_host(), ref, tag + ", y = A x")
        y0 = self.rng.integers(1, 9, size=rows).astype(np.float64)
        y0[np.flatnonzero(self.empty)[::2]] = -0.0         # an untouched -0.0 stays -0.0; one that got `+ 0.0` is +0.0
        ref_acc = np.where(self.empty, y0, (exact + y0.astype(np.int64)).astype(np.float64))
        assert np.array_equal(bits(oracle_spmv(self.shape, self.ip, self.ix, self.dt, x, y=y0)), bits(ref_acc)), tag + ": oracle, y += A x"
        yv = DeviceVec.from_host(y0)
        prod.mul_acc_mat_vec_csr(self.a, xv, yv, stream=stream)
        if stream is not None:
            stream.synchronize()
        assert self.a.spmv_plan_info()[0] == kind
        self.same(yv.to_host(), ref_acc, tag + ", y += A x")


def check_random(hip, shape, ip, ix, kind, seed=0):
    """one round of random doubles against the oracle (the float path has its own roundings), both forms"""
    from sprs_amd import prod
    from sprs_amd.device import DeviceCsMat, DeviceVec
    rng = np.random.default_rng(seed + 77)
    dt = rng.random(ix.size) + 0.5
    x = rng.random(shape[1]) + 0.5
    empty = np.diff(ip.astype(np.int64)) == 0
    a = DeviceCsMat.from_host(shape, ip, ix, dt)
    xv = DeviceVec.from_host(x)
    y = (a * xv).to_host()
    assert a.spmv_plan_info()[0] == kind
    assert rel_err(y, oracle_spmv(shape, ip, ix, dt, x)) <= TOL
    assert np.array_equal(bits(y[empty]), bits(np.zeros(int(empty.sum()))))
    y0 = rng.random(shape[0]) + 0.5
    yv = DeviceVec.from_host(y0)
    prod.mul_acc_mat_vec_csr(a, xv, yv)
    assert a.spmv_plan_info()[0] == kind
    y2 = yv.to_host()
    assert rel_err(y2, oracle_spmv(shape, ip, ix, dt, x, y=y0)) <= TOL
    assert np.array_equal(bits(y2[empty]), bits(y0[empty]))


def check_exact(hip, shape, ip, ix, tile, kind, seed=0):
    """three exact rounds on one handle"""
    ex = Exact(hip, shape, ip, ix, tile, seed=seed)
    for _ in range(3):
        ex.round(kind)
    return ex


def check_seam(hip, shape, ip, ix, tile, kind, seed=0):
    """a seam case: the exact rounds, and one round of random doubles"""
    check_exact(hip, shape, ip, ix, tile, kind, seed=seed)
    check_random(hip, shape, ip, ix, kind, seed=seed)


# ---------------------------------------------------------------------------------------------
# A. the plain tile plan (spmv_xcs = 2).  Cases as row lengths, functions of the tile T.
# ---------------------------------------------------------------------------------------------
PLAIN = {
    # A1: the full-tile vector path against the guarded partial path, an odd count in the last tile included
    "a1-T": lambda T: [T],
    "a1-T-1,1": lambda T: [T - 1, 1],
    "a1-T+1": lambda T: [T + 1],
    "a1-T,T": lambda T: [T, T],
    "a1-2T-1": lambda T: [2 * T - 1],
    "a1-1": lambda T: [1],
    # A2: row ends and starts on a tile edge (tile_row is a lower bound on indptr; carry_body returns early)
    "a2-empty-run-on-edge": lambda T: [1, T - 1, 0, 0, 0, T, 1, 0],
    "a2-span-ends-on-edge": lambda T: [T, 2 * T, 0, 7],
    "a2-carry-over-three-tiles": lambda T: [5, 3 * T + 5, 0, 0, 2],
    "a2-two-spans": lambda T: [T - 1, 3 * T, T + 1],
    # A3: more row starts in one tile than SEG_CHUNK (the j0 loop: nlong reset between chunks, longlist indexed per chunk)
    "a3-empty-rows-around-T": lambda T: [0] * 5000 + [T] + [0] * 5000 + [3],
    "a3-long-in-second-chunk": lambda T: [1] * 2048 + [100] + [1] * 1000 + [70],     # 3218 entries: one tile at T = 4096
    # (a long row in the FIRST chunk too: were nlong not reset, its list slot t = 1 would be read again in the second chunk,
    # where it names row 2048, a row of one entry, which the accumulate form would then add twice)
    "a3-long-in-both-chunks": lambda T: [100] + [0, 1] * 1100 + [70] + [1] * 50,
    "a3-S-2048": lambda T: [1] * 2046 + [65],
    "a3-S-2049": lambda T: [1] * 2047 + [65],
    # A4: LONG_SEG and the capacity of longlist; the head segment (j == 0) by the lane path and by the wave path
    "a4-longlist-full": lambda T: [64] * (T // 64) + [63, 65],
    "a4-head-63": lambda T: [7, T + 56, 9],
    "a4-head-64": lambda T: [7, T + 57, 9],
    "a4-head-T": lambda T: [7, 3 * T - 7, 9],
    # A5: the accumulate form on every kind of segment: short, long, empty, head only, a row that is only a head in its last tile
    "a5-every-segment-kind": lambda T: [10, 70, 0, T, 0, 2 * T + 5, 0, 63, 64, 0],
    "a5-head-only-last-tile": lambda T: [3, 0, T + 40],
}


def plain_params(cases):
    out = []
    for name, f in cases.items():
        for T in TILES:
            for idx, ptr in (W4 if sum(f(T)) >= 2 * T else W2):
                out.append(pytest.param(name, T, idx, ptr, id="%s-%d-%s" % (name, T, wname(idx, ptr))))
    return out


@pytest.mark.parametrize("name,T,idx,ptr", plain_params(PLAIN))
def test_plain_tile_seams(hip, name, T, idx, ptr):
    """A1 - A5: see the table above"""
    lens = PLAIN[name](T)
    shape, ip, ix = seam_csr(lens, seed=len(lens) + T, idx=idx, ptr=ptr)
    if name == "a3-long-in-second-chunk" and T == 4096:
        assert ix.size <= T                                     # one tile: both long rows belong to its second chunk
    with spmv_options(hip, spmv_xcs=2, spmv_tile=T):
        check_seam(hip, shape, ip, ix, T, 1, seed=T)


@pytest.mark.parametrize("T,idx,ptr,ntiles", [pytest.param(T, i, p, n, id="%d-%s-%d" % (T, wname(i, p), n)) for T in TILES
                                              for n in (1, 7, 8, 9, 15, 16, 17) for i, p in (W4 if n >= 2 else W2)])
def test_tile_of_block(hip, T, idx, ptr, ntiles):
    """A6: blockIdx -> tile for tile counts around the multiples of 8, rows of 37 entries so that the edges fall inside rows.
    The accumulate form sees a tile done twice, the poisoned y one not done."""
    n = ntiles * T // 37
    assert (ntiles - 1) * T < 37 * n <= ntiles * T
    shape, ip, ix = seam_csr([37] * n, cols=900, seed=ntiles, idx=idx, ptr=ptr)
    with spmv_options(hip, spmv_xcs=2, spmv_tile=T):
        check_seam(hip, shape, ip, ix, T, 1, seed=ntiles)


@device_only
@pytest.mark.parametrize("idx,ptr", W4, ids=[wname(i, p) for i, p in W4])
@pytest.mark.parametrize("T", TILES)
def test_second_workgroup_of_the_plan_kernels(hip, T, idx, ptr):
    """A7: 259 tiles — build_tile_rows and spmv_carry_kernel run one thread per tile in workgroups of 256; a row that starts in
    tile 256 and runs through tiles 257 and 258 has its carries added by a thread of the second workgroup"""
    n1 = (256 * T + 50) // 37 + 1
    lens = [37] * n1 + [2 * T + 11]
    n2 = (258 * T + 100 - sum(lens)) // 37
    lens += [37] * n2 + [0, 5]
    start = 37 * n1
    assert 256 * T < start < 257 * T and start + 2 * T + 11 > 258 * T and -(-sum(lens) // T) == 259
    shape, ip, ix = seam_csr(lens, cols=3 * T, seed=T, idx=idx, ptr=ptr)
    with spmv_options(hip, spmv_xcs=2, spmv_tile=T):
        check_seam(hip, shape, ip, ix, T, 1, seed=T)


@device_only
@pytest.mark.parametrize("idx,ptr", W4, ids=[wname(i, p) for i, p in W4])
def test_row_wave_kernel_grid_stride(hip, idx, ptr):
    """A7: the one-wave-per-row kernel with more rows than the 256 * 32 * 4 = 32768 waves of its largest grid: the grid-stride
    loop is entered, with rows of 0, 1, 63, 64, 65 and 129 entries in front of and behind that row.  No plan is built: kind 0."""
    rows = 33001
    lens = np.tile([0, 1, 2, 1], rows // 4 + 1)[:rows]
    for k, v in enumerate((63, 64, 65, 129)):
        lens[k::97] = v
    assert set(lens[32768:].tolist()) >= {0, 1, 63, 64, 65, 129}
    shape, ip, ix = seam_csr(lens, cols=5000, seed=3, idx=idx, ptr=ptr)
    with spmv_options(hip, spmv_kernel=2, spmv_xcs=2):
        check_seam(hip, shape, ip, ix, 4096, 0, seed=3)


def split_rows(T):
    """B1's matrix: rows of split - 1, split and split + 1 entries (split = 64) interleaved, one row of 5 T + 3, empty rows"""
    lens = [63, 64, 0, 65] * 150 + [5 * T + 3] + [65, 63, 0, 64] * 150 + [0, 0]
    return lens, 5 * T + 3 + 4000


def x_slice(col):
    """spmv_shared.hpp x_slice restated: the top 3 bits of a multiplicative hash of the column's 128-byte line number"""
    return ((np.asarray(col, dtype=U64) >> U64(4)) * U64(0x9E3779B97F4A7C15)) >> U64(61)


def test_plan_follows_the_options(hip):
    """A8: one handle multiplies at T = 2048, then at T = 4096, then under spmv_xcs = 1 with a split that makes long rows: the
    plan is rebuilt each time (kinds 1, 1, 2) and the bits stay the oracle's"""
    lens, cols = split_rows(2048)
    shape, ip, ix = seam_csr(lens, cols=cols, seed=8)
    with spmv_options(hip, spmv_xcs=2, spmv_tile=2048):
        ex = Exact(hip, shape, ip, ix, 2048, seed=8)
        ex.round(1)
        hip.set_option("spmv_tile", 4096)
        ex.tile = 4096
        ex.round(1)
        hip.set_option("spmv_xcs", 1)
        hip.set_option("spmv_xcs_split", 64)
        ex.round(2)
        ex.round(2)


@pytest.mark.parametrize("T", TILES)
def test_prepare_builds_the_sliced_plan_at_once(hip, T):
    """A8: prepare() before the first multiply gives the sliced plan (kind 2) at once, and the multiplies run on it"""
    lens, cols = split_rows(T)
    shape, ip, ix = seam_csr(lens, cols=cols, seed=9)
    with spmv_options(hip, spmv_xcs=1, spmv_xcs_split=64, spmv_tile=T):
        ex = Exact(hip, shape, ip, ix, T, seed=9)
        assert ex.a.spmv_plan_info()[0] == 0
        ex.a.prepare()
        assert ex.a.spmv_plan_info()[0] == 2
        ex.round(2)
        ex.round(2)
        check_random(hip, shape, ip, ix, 2, seed=9)


@pytest.mark.parametrize("T", TILES)
@pytest.mark.parametrize("idx,ptr", W4, ids=[wname(i, p) for i, p in W4])
def test_host_one_shot_carries(hip, T, idx, ptr):
    """A8: the host one-shot entry (plain tiles whatever spmv_xcs says) on the row that carries over three later tiles"""
    from sprs_amd import _ffi
    lens = [5, 3 * T + 5, 0, 0, 2]
    shape, ip, ix = seam_csr(lens, seed=T, idx=idx, ptr=ptr)
    rows, cols = shape
    rng = np.random.default_rng(T)
    dt = rng.integers(1, 5, size=ix.size).astype(np.float64)
    x = (rng.permutation(cols) + 1).astype(np.float64)
    exact = int64_spmv(ip, ix, dt, x)
    assert exact.max() + 8 < 2 ** 53
    vp = lambda a: C.c_void_p(a.ctypes.data)
    helpers.fresh_blocks()
    with spmv_options(hip, spmv_xcs=1, spmv_xcs_split=64, spmv_tile=T):
        for acc in (1, 0):
            y0 = np.array([3.0, 5.0, -0.0, 2.0, 7.0])
            ref = np.where(np.array(lens) == 0, y0, exact + y0) if acc else exact.astype(np.float64)
            assert np.array_equal(bits(oracle_spmv(shape, ip, ix, dt, x, y=y0 if acc else None)), bits(ref))
            y = y0.copy() if acc else np.full(rows, np.nan)
            _ffi.check(_ffi.lib.sprs_hip_spmv_f64_host(rows, cols, vp(ip), ip.dtype.itemsize, vp(ix), ix.dtype.itemsize, vp(dt),
                                                       vp(x), cols, vp(y), rows, acc))
            assert np.array_equal(bits(y), bits(ref)), (acc, y.tolist(), ref.tolist())


# ---------------------------------------------------------------------------------------------
# B. the XCD-sliced plan (spmv_xcs = 1): classify, fill, count, scatter, per-slice tiles and carries, the reduce over 8 partials,
#    the column relabelling, the per-tile column sort
# ---------------------------------------------------------------------------------------------
COMBOS = [(r, s, i) for r in (1, 2) for s in (0, 1) for i in (0, 1)]


def combo_params(widths=W2):
    return [pytest.param(T, idx, ptr, r, s, i, id="%d-%s-relabel%d-sort%d-idx32_%d" % (T, wname(idx, ptr), r, s, i))
            for T in TILES for idx, ptr in widths for r, s, i in COMBOS]


@pytest.mark.parametrize("T,idx,ptr,relabel,srt,idx32", combo_params())
def test_split_threshold(hip, T, idx, ptr, relabel, srt, idx32):
    """B1: rows of split - 1, split and split + 1 entries, a row of 5 T + 3 and empty rows; the short piece and (in the natural
    labelling, by the restated hash) every slice have more than one tile"""
    lens, cols = split_rows(T)
    shape, ip, ix = seam_csr(lens, cols=cols, seed=T + 1, idx=idx, ptr=ptr)
    lens = np.asarray(lens)
    long_entry = np.repeat(lens >= 64, lens)
    assert lens[lens < 64].sum() > T and np.bincount(x_slice(ix[long_entry]).astype(np.int64), minlength=8).min() > T
    with spmv_options(hip, spmv_xcs=1, spmv_xcs_split=64, spmv_tile=T, spmv_relabel=relabel, spmv_sort_tiles=srt, spmv_xcs_idx32=idx32):
        check_seam(hip, shape, ip, ix, T, 2, seed=T + relabel)


@pytest.mark.parametrize("T,idx,ptr,relabel,srt,idx32", combo_params())
def test_no_short_rows(hip, T, idx, ptr, relabel, srt, idx32):
    """B2: every stored row is long: the short piece has no tile, so the operator form must zero the empty rows itself and the
    accumulate form must leave them alone, -0.0 included"""
    lens = [64, 0, 70, 0, 0, 3 * T]
    shape, ip, ix = seam_csr(lens, seed=T + 2, idx=idx, ptr=ptr)
    with spmv_options(hip, spmv_xcs=1, spmv_xcs_split=64, spmv_tile=T, spmv_relabel=relabel, spmv_sort_tiles=srt, spmv_xcs_idx32=idx32):
        check_seam(hip, shape, ip, ix, T, 2, seed=T + relabel)


@pytest.mark.parametrize("T,idx,ptr,relabel,srt,idx32", combo_params())
def test_no_long_rows(hip, T, idx, ptr, relabel, srt, idx32):
    """B3: no row reaches the split: the plan falls back to the plain tiles (kind 1) and is still exact"""
    shape, ip, ix = seam_csr([5, 6, 7, 0], cols=300, seed=T + 3, idx=idx, ptr=ptr)
    with spmv_options(hip, spmv_xcs=1, spmv_xcs_split=64, spmv_tile=T, spmv_relabel=relabel, spmv_sort_tiles=srt, spmv_xcs_idx32=idx32):
        check_seam(hip, shape, ip, ix, T, 1, seed=T + relabel)


@pytest.mark.parametrize("relabel", [1, 2])
@pytest.mark.parametrize("idx,ptr", W2, ids=[wname(i, p) for i, p in W2])
@pytest.mark.parametrize("T", TILES)
def test_slices_without_entries(hip, T, idx, ptr, relabel):
    """B4: 300 rows that each store exactly the columns 32 .. 47 — one x line, so every entry lands in ONE slice whatever the
    hash is (with the relabelling the sixteen columns are the top class and stay one line).  That slice has more than one tile;
    the other seven launch nothing, and their partial sums must read as zero."""
    rows, cols = 300, 100
    ip = (16 * np.arange(rows + 1)).astype(ptr)
    ix = np.tile(np.arange(32, 48), rows).astype(idx)
    assert ix.size > T
    with spmv_options(hip, spmv_xcs=1, spmv_xcs_split=16, spmv_tile=T, spmv_relabel=relabel):
        check_seam(hip, (rows, cols), ip, ix, T, 2, seed=T + relabel)


@pytest.mark.parametrize("idx,ptr", W2, ids=[wname(i, p) for i, p in W2])
@pytest.mark.parametrize("T", TILES)
def test_long_row_spanning_tiles_inside_one_slice(hip, T, idx, ptr):
    """B5: natural labelling; a row of 70 and a row of 3 T entries whose columns all hash to ONE slice (chosen with x_slice
    above, the restatement of the kernel's hash — if the hash changes, the assertion below fails and the case no longer covers
    this): the long row spans four tiles of that slice, so the sliced carry kernel adds three carries, with max_tiles taken from
    this slice while the other seven return at tile >= ntiles.  A short row and an empty row beside them."""
    cols = 131072
    lines = np.arange(cols // 16, dtype=np.int64)
    mine = lines[x_slice(16 * lines) == U64(5)]
    assert mine.size * 16 >= 3 * T + 70
    ids = (16 * mine[:, None] + np.arange(16)[None, :]).ravel()
    lens = [5, 70, 0, 3 * T]
    pins = [(1, ids[-70:]), (3, ids[:3 * T])]
    shape, ip, ix = seam_csr(lens, cols=cols, seed=T + 5, idx=idx, ptr=ptr, pins=pins)
    assert set(x_slice(ix[5:]).tolist()) == {5}
    with spmv_options(hip, spmv_xcs=1, spmv_xcs_split=64, spmv_tile=T, spmv_relabel=2):
        check_seam(hip, shape, ip, ix, T, 2, seed=T + 5)


COUNTS = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 11, 12, 16])       # the half-octave edges of rl_digit, and never referenced


@pytest.mark.parametrize("cols", [1023, 1024, 1025, 2049])
@pytest.mark.parametrize("idx,ptr", W2, ids=[wname(i, p) for i, p in W2])
@pytest.mark.parametrize("T", TILES)
def test_relabelling_at_the_class_and_chunk_edges(hip, T, idx, ptr, cols):
    """B6: column j is referenced COUNTS[j % 12] times (the counts on both sides of every half-octave edge up to 16; a twelfth
    of the columns never — they are the last class, and rl_permute_x_kernel must still write every slot of the permuted x),
    the references dealt to the rows round-robin so that rows of split - 1, split and split + 1 entries exist; cols around
    RL_CHUNK = 1024 and one column into a third chunk"""
    want = COUNTS[np.arange(cols) % COUNTS.size]
    col = np.repeat(np.arange(cols), want)
    nrows = col.size // 64
    row = np.arange(col.size) % nrows                            # a column's references go to consecutive rows: distinct
    order = np.lexsort((col, row))
    ix = col[order].astype(idx)
    lens = np.bincount(row, minlength=nrows)
    ip = np.zeros(nrows + 1, dtype=np.int64)
    np.cumsum(lens, out=ip[1:])
    assert np.array_equal(np.bincount(ix.astype(np.int64), minlength=cols), want)
    assert all(np.all(np.diff(ix[ip[r]:ip[r + 1]].astype(np.int64)) > 0) for r in (0, nrows // 2, nrows - 1))
    split = int(lens.max())
    assert (lens >= split).sum() >= 3 and (lens < split).sum() >= 3
    with spmv_options(hip, spmv_xcs=1, spmv_xcs_split=split, spmv_tile=T, spmv_relabel=1):
        check_seam(hip, (nrows, cols), ip.astype(ptr), ix, T, 2, seed=cols)


@device_only
@pytest.mark.parametrize("idx,ptr", W2, ids=[wname(i, p) for i, p in W2])
@pytest.mark.parametrize("T", TILES)
def test_grid_stride_loops_of_the_plan_build(hip, T, idx, ptr):
    """B7: 66 000 rows of 16 entries at split 16 — more long rows than the 65 536 waves of xcs_count_kernel's and
    xcs_scatter_kernel's largest grid, more than one block of xcs_reduce_kernel, more entries than the 1 048 576 threads of
    rl_count_kernel; rows whose lengths are no multiple of 64 (the lane validity of count and scatter) and short rows between"""
    lens = np.full(66000, 16)
    lens[::9001] = (17, 70, 100, 130, 3, 0, 64, 129)
    lens[65990:] = (17, 70, 3, 0, 130, 16, 16, 100, 0, 65)
    assert (lens >= 16).sum() > 65536 and 1048576 < lens.sum() < 1100000
    shape, ip, ix = seam_csr(lens, cols=70000, seed=T + 7, idx=idx, ptr=ptr)
    with spmv_options(hip, spmv_xcs=1, spmv_xcs_split=16, spmv_tile=T):
        check_seam(hip, shape, ip, ix, T, 2, seed=T + 7)


@device_only
@pytest.mark.parametrize("T", TILES)
def test_two_streams_one_handle(hip, T):
    """B8: the plan keeps one scratch per stream (carries, partials, permuted x, the argument table): the null stream, a
    non-blocking torch stream, the null stream again, both forms, exact every time"""
    import torch
    s = torch.cuda.Stream(device=torch.device("cuda", 0))
    lens, cols = split_rows(T)
    shape, ip, ix = seam_csr(lens, cols=cols, seed=T + 8)
    with spmv_options(hip, spmv_xcs=1, spmv_xcs_split=64, spmv_tile=T):
        ex = Exact(hip, shape, ip, ix, T, seed=T + 8)
        for stream in (None, s, None, s):
            ex.round(2, stream=stream)
