"""The BANDED SpMV plan on f32 handles (sprs_amd/csrc/spmv_band.hip with float values, x, partial sums and carries; hot slices
of 8192, 16384 or 32768 labels: option spmv_f32_band_tile).  Every case asserts that the product ran on the banded plan
(spmv_plan_info()[0] == 3), takes every product twice and compares the bits run to run, and runs the operator and the accumulate
form on ONE handle over two different x — a stale partial sum, carry or permuted-x slot of the first product shows in the second.

EXACT cases: values and x are integers 1 .. 4, y0 integers 1 .. 8.  A product is at most 16, so every sum of a row of up to 2^20
entries stays below 2^24 and is exact in f32 in ANY order of additions: the bits of tests/f32_ref.py (the reference's left-to-right
chain) are the only right answer, whatever order the plan adds in.
ROUNDED cases: the per-row forward bound of tests/test_f32_gpu.py — |y - s| <= gamma_m sum |a x| for the operator form, gamma_{m+1}
for the accumulate form, plus the float64 reference sum's own slack m 2^-52 sum |a x| — which holds for any order of m - 1 f32
additions of rounded products.

The same file runs through the kernel emulator on the CPU (tests/test_spmv_band_f32_emu_cpu.py)."""
import os

import numpy as np
import pytest

import f32_ref
from helpers import ragged_csr

pytestmark = pytest.mark.gpu

EMULATED = bool(os.environ.get("SPRS_HIP_LIBRARY"))     # the kernel emulator of tests/emu: its device memory is host memory
WIDTHS = [(np.uint32, np.uint32), (np.uint32, np.uint64), (np.uint64, np.uint32), (np.uint64, np.uint64)]   # (indices, indptr)
U = 2.0 ** -24


@pytest.fixture(scope="module")
def hip():
    import sprs_amd
    if sprs_amd.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X (no CPU fallback exists)")
    return sprs_amd


class band_options:
    def __init__(self, hip, **vals):
        self.hip, self.vals = hip, dict(spmv_band=1, **vals)

    def __enter__(self):
        for k, v in self.vals.items():
            self.hip.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.vals:
            self.hip.set_option(k, 0)


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def small_ints(n, hi, seed):
    return np.random.default_rng(seed).integers(1, hi + 1, size=n).astype(np.float32)


def products(hip, a, xs, y0, mul_acc=None):
    """[(y = A x, y0 + A x) for x in xs] on the handle `a`, which must run on the banded plan; every product is taken twice and
    must give the same bits, and after the last x the first is taken again (nothing of the products in between may be left)"""
    from sprs_amd import prod
    from sprs_amd.device import DeviceVecF32
    mul_acc = mul_acc or prod.mul_acc_mat_vec_csr
    out = []
    for x in xs:
        xv = DeviceVecF32.from_host(x)
        y = (a * xv).to_host()
        kind, nbytes = a.spmv_plan_info()
        assert kind == 3 and nbytes > 0                         # (a case that falls back to the tile plan tests nothing)
        assert y.dtype == np.float32 and bits(y) == bits((a * xv).to_host())
        acc = []
        for _ in range(2):
            yv = DeviceVecF32.from_host(y0)
            mul_acc(a, xv, yv)
            acc.append(yv.to_host())
        assert bits(acc[0]) == bits(acc[1])
        out.append((y, acc[0]))
    assert bits((a * DeviceVecF32.from_host(xs[0])).to_host()) == bits(out[0][0])
    assert a.spmv_plan_info() == (3, nbytes)
    return out


class Exact:
    """an integer-valued matrix with its two x, y0 and the reference's bits, computed once and shared by the cases that use it"""

    def __init__(self, shape, ip, ix, seed=0, dt=None, xs=None):
        self.shape, self.ip, self.ix = shape, ip, ix
        self.dt = small_ints(ix.size, 4, seed) if dt is None else dt
        self.xs = [small_ints(shape[1], 4, seed + 1), small_ints(shape[1], 4, seed + 2)] if xs is None else xs
        self.y0 = small_ints(shape[0], 8, seed + 3)
        with np.errstate(all="ignore"):
            self.want = [(f32_ref.mul_vec(shape, ip, ix, self.dt, x), f32_ref.mul_acc_mat_vec_csr(shape, ip, ix, self.dt, x, self.y0.copy()))
                         for x in self.xs]
        self.empty = np.diff(ip.astype(np.int64)) == 0

    def compare(self, got):
        for (y, acc), (wy, wacc) in zip(got, self.want):
            nan = np.isnan(wy)
            assert np.array_equal(np.isnan(y), nan) and np.array_equal(np.isnan(acc), np.isnan(wacc))
            assert bits(y[~nan]) == bits(wy[~nan]) and bits(acc[~nan]) == bits(wacc[~nan])
            assert bits(y[self.empty]) == bits(np.zeros(int(self.empty.sum()), dtype=np.float32))     # +0.0f
            assert bits(acc[self.empty]) == bits(self.y0[self.empty])

    def check(self, hip, idx=None, ptr=None, **opts):
        from sprs_amd.device import DeviceCsMatF32
        ip = self.ip if ptr is None else self.ip.astype(ptr)
        ix = self.ix if idx is None else self.ix.astype(idx)
        with band_options(hip, **opts):
            a = DeviceCsMatF32.from_host(self.shape, ip, ix, self.dt)
            assert a.spmv_plan_info()[0] == 0
            self.compare(products(hip, a, self.xs, self.y0))
        return a


# ---- case 1: every index-width pair, every slice width -----------------------------------------------------------------------
def long_rows_lengths(rows=260, seed=0):
    """long rows of 40 .. 200 entries between empty rows and rows of one entry (short at split 2)"""
    lens = np.random.default_rng(seed).integers(40, 200, size=rows)
    lens[::9] = 0
    lens[4::11] = 1
    return [int(v) for v in lens]


@pytest.fixture(scope="module")
def long_rows():
    shape, ip, ix, _ = ragged_csr(long_rows_lengths(), 20000, seed=0, idx=np.uint32, ptr=np.uint32)
    return Exact(shape, ip, ix, seed=10)


# 20 000 columns: three slices of 8192 labels, two of 16384 or one of 32768 cover them
TILES = [(8192, 3), (16384, 2), (32768, 1)]


@pytest.mark.parametrize("tile,hot", TILES)
@pytest.mark.parametrize("idx,ptr", WIDTHS)
def test_every_index_width_and_slice_width(hip, long_rows, idx, ptr, tile, hot):
    long_rows.check(hip, idx=idx, ptr=ptr, spmv_f32_band_tile=tile, spmv_band_hot=hot, spmv_band_split=2)


# ---- case 2: slices of 1, 511, 512, 513, 1025 entries -------------------------------------------------------------------------
def seam_matrix(n):
    """8192 + n columns referenced once each (one popularity class: labels in column order), rows of 64: slice 0 of 8192 labels holds
    8192 entries = 16 tiles, slice 1 exactly n"""
    total = 8192 + n
    lens = [64] * (total // 64 - 1) + [64 + total % 64]
    ip = np.zeros(len(lens) + 1, dtype=np.uint32)
    ip[1:] = np.cumsum(lens)
    return (len(lens), 3 * total), ip, (3 * np.arange(total)).astype(np.uint32)


@pytest.mark.parametrize("n", [1, 511, 512, 513, 1025])
def test_slice_sizes_at_the_tile_seams(hip, n):
    shape, ip, ix = seam_matrix(n)
    Exact(shape, ip, ix, seed=n).check(hip, spmv_f32_band_tile=8192, spmv_band_hot=2, spmv_band_split=2, spmv_band_hot_run=1)


# ---- case 3: hub rows over many segments ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hubs():
    lens = [0, 20000, 3, 0] + [33] * 700 + [20000] + [1, 0, 31, 32] * 20 + [33] * 700 + [20000, 0, 0, 7]
    shape, ip, ix, _ = ragged_csr(lens, 20000, seed=3, idx=np.uint32, ptr=np.uint32)
    return Exact(shape, ip, ix, seed=30)


@pytest.mark.parametrize("overlap,tail", [(1, 0), (1, 2), (2, 0), (2, 2)])
@pytest.mark.parametrize("rounds,tile,hot,run", [(1, 8192, 2, 0), (3, 16384, 2, 1), (40, 8192, 3, 3), (2, 32768, 1, 1000)])
def test_hub_rows_over_many_segments(hip, hubs, rounds, tile, hot, run, overlap, tail):
    """three dense rows (every slice sees rows that span several tiles, ranges and workgroups: register carries, head carries, runs of
    ranges without a row start) between rows of 33 entries, under one to forty hot workgroups per CU and ranges of one tile up to a
    whole segment; the gather launches on the second stream or on the caller's, the short rows in the reduction's launch or alone"""
    hubs.check(hip, spmv_f32_band_tile=tile, spmv_band_hot=hot, spmv_band_rounds=rounds, spmv_band_hot_run=run, spmv_band_phases=2,
               spmv_band_overlap=overlap, spmv_band_tail=tail)


# ---- case 4: a 32768-label slice addressed past 16383 -----------------------------------------------------------------------------
def test_slice_of_32768_labels_uses_id_bit_14(hip):
    """40 000 columns referenced twice each, rows of 64.  Every column is referenced, so slice 0 holds entries under each of its
    32768 labels, whichever column got which label: local ids 16384 .. 32767 (bit 14 of the raw id, the key selector of packed f64
    slices) are in use, and slice 1 takes the remaining 7232 labels"""
    cols = 40000
    rng = np.random.default_rng(4)
    ix = np.concatenate([np.sort(rng.permutation(cols).reshape(-1, 64), axis=1).ravel() for _ in range(2)]).astype(np.uint32)
    ip = (64 * np.arange(ix.size // 64 + 1)).astype(np.uint32)
    assert np.unique(ix).size == cols > 32768 + 512            # labels 16384 .. 32767 of slice 0 all carry entries
    Exact((ip.size - 1, cols), ip, ix, seed=40).check(hip, spmv_f32_band_tile=32768, spmv_band_hot=2, spmv_band_split=2)


# ---- case 5: tiles full of row starts, cold rest in several phases ----------------------------------------------------------------
def test_tiles_full_of_row_starts_and_a_cold_rest_in_phases(hip):
    """rows of 2 entries (long at split 2) over 32768 columns referenced once each, with a few rows of 700: a hot tile of such rows
    holds up to 512 row starts — four passes of the 128-slot staging window — and the hot band (two slices of 8192 labels) covers
    half the columns, so the other half of the entries is the cold rest: 8 hash pieces in each of 2 label ranges"""
    cols = 32768
    rng = np.random.default_rng(5)
    perm = rng.permutation(cols)
    lens = [2] * 3000 + [700, 0, 1, 700] + [2] * ((cols - 6000 - 1401) // 2)
    lens.append(cols - sum(lens))
    ip = np.zeros(len(lens) + 1, dtype=np.uint32)
    ip[1:] = np.cumsum(lens)
    ix = np.concatenate([np.sort(perm[int(ip[r]):int(ip[r + 1])]) for r in range(len(lens))]).astype(np.uint32)
    assert ix.size == cols and lens.count(2) > 10000
    Exact((len(lens), cols), ip, ix, seed=50).check(hip, spmv_f32_band_tile=8192, spmv_band_hot=2, spmv_band_split=2, spmv_band_phases=2)


# ---- case 6: specials --------------------------------------------------------------------------------------------------------------
def test_infinite_x_at_a_padded_slices_first_label(hip):
    """slice 1 of the seam matrix with n = 513 ends in a tile of one entry and 511 padding slots (value 0, id 0 = the slice's first
    label, column 3 x 8192): x = +Inf there reaches exactly the one row that references the column; a padding product 0 x Inf would
    put a NaN into the last row"""
    shape, ip, ix = seam_matrix(513)
    xs = [small_ints(shape[1], 4, 61), small_ints(shape[1], 4, 62)]
    xs[0][3 * 8192] = np.inf
    xs[1][0] = np.inf                                           # slice 0's first label: 16 full tiles, no padding
    ex = Exact(shape, ip, ix, seed=60, xs=xs)
    assert np.isinf(ex.want[0][0]).sum() == 1 and not np.isnan(ex.want[0][0]).any()
    ex.check(hip, spmv_f32_band_tile=8192, spmv_band_hot=2, spmv_band_split=2, spmv_band_hot_run=1)


def test_zeros_and_denormals(hip, long_rows):
    """+-0.0 and f32 denormals down to the smallest, x integers 1 .. 4: every product is a multiple of 2^-149 of at most 4e-41, and
    a row of up to 200 of them sums to at most 8e-39 < 2^-126 — below the normal range, where the spacing of floats IS 2^-149 —,
    hence every sum is exact in any order"""
    rng = np.random.default_rng(6)
    pool = np.array([0.0, -0.0, 1e-45, -1e-45, 1.4e-44, -7e-43, 1e-41], dtype=np.float32)
    assert pool[2] > 0 and np.signbit(pool[1]) and 200 * 4 * float(np.abs(pool).max()) < 2.0 ** -126
    dt = pool[rng.integers(0, pool.size, size=long_rows.ix.size)]
    Exact(long_rows.shape, long_rows.ip, long_rows.ix, seed=63, dt=dt).check(hip, spmv_f32_band_tile=8192, spmv_band_hot=3, spmv_band_split=2)


# ---- case 7: CSC handles and refresh ---------------------------------------------------------------------------------------------
def test_csc_handle_runs_on_its_csr_forms_plan(hip, long_rows):
    from sprs_amd import _ffi, prod
    from sprs_amd.device import DeviceCsMatF32
    ex = long_rows
    _, cp, ci, cd = f32_ref.csc_to_csr(ex.shape[::-1], ex.ip, ex.ix, ex.dt)      # the CSC arrays of the same matrix
    with band_options(hip, spmv_f32_band_tile=16384, spmv_band_hot=2, spmv_band_split=2):
        a = DeviceCsMatF32.from_host(ex.shape, cp.astype(np.uint32), ci.astype(np.uint32), cd, storage=_ffi.CSC)
        assert a.spmv_plan_info()[0] == 0
        ex.compare(products(hip, a, ex.xs, ex.y0, mul_acc=prod.mul_acc_mat_vec_csc))


def test_values_changed_in_place_and_refresh_rebuild_the_plan(hip, long_rows):
    import torch
    from sprs_amd.device import DeviceCsMatF32
    ex = long_rows
    dev = "cpu" if EMULATED else "cuda"
    tip, tix, tdt = [torch.from_numpy(a.astype(np.int32) if a.dtype != np.float32 else a.copy()).to(dev) for a in (ex.ip, ex.ix, ex.dt)]
    opts = dict(spmv_f32_band_tile=8192, spmv_band_hot=3, spmv_band_split=2)
    with band_options(hip, **opts):
        a = DeviceCsMatF32.wrap_torch(ex.shape, tip, tix, tdt)
        ex.compare(products(hip, a, ex.xs, ex.y0))
        nbytes = a.spmv_plan_info()[1]
        tdt.mul_(2.0)                                           # integers 2 .. 8: sums still far below 2^24
        tdt[::5] = 1.0
        if not EMULATED:
            torch.cuda.synchronize()
        a.refresh()
        assert a.spmv_plan_info()[0] == 0
        dt2 = 2.0 * ex.dt
        dt2[::5] = 1.0
        ex2 = Exact(ex.shape, ex.ip, ex.ix, seed=10, dt=dt2.astype(np.float32))
        got = products(hip, a, ex2.xs, ex2.y0)
        ex2.compare(got)
        assert a.spmv_plan_info() == (3, nbytes)
        fresh = products(hip, DeviceCsMatF32.from_host(ex.shape, ex.ip, ex.ix, ex2.dt), ex2.xs, ex2.y0)
        assert all(bits(g[0]) == bits(f[0]) and bits(g[1]) == bits(f[1]) for g, f in zip(got, fresh))


# ---- rounded arithmetic --------------------------------------------------------------------------------------------------------
def check_bound(hip, shape, ip, ix, dt, seed):
    """the bound of tests/test_f32_gpu.py::_check_bound for both forms and two x, on one banded handle"""
    from sprs_amd.device import DeviceCsMatF32
    rng = np.random.default_rng(seed)
    ip64 = ip.astype(np.int64)
    m = np.diff(ip64).astype(np.float64)
    xs = [((rng.random(shape[1]) + 0.5) * rng.choice([-1.0, 1.0], size=shape[1])).astype(np.float32) for _ in range(2)]
    y0 = ((rng.random(shape[0]) + 0.5) * rng.choice([-1.0, 1.0], size=shape[0])).astype(np.float32)
    a = DeviceCsMatF32.from_host(shape, ip, ix, dt)
    got = products(hip, a, xs, y0)
    gamma = m * U / (1.0 - m * U)
    gamma1 = (m + 1) * U / (1.0 - (m + 1) * U)
    empty = m == 0
    for x, (y, ya) in zip(xs, got):
        p = dt.astype(np.float64) * x.astype(np.float64)[ix.astype(np.int64)]
        # per-row sums in float64 (reduceat on a padded array: an empty row reads one element, zeroed below)
        S = np.where(m > 0, np.add.reduceat(np.concatenate([np.abs(p), [0.0]]), ip64[:-1]), 0.0)
        s = np.where(m > 0, np.add.reduceat(np.concatenate([p, [0.0]]), ip64[:-1]), 0.0)
        slack = m * 2.0 ** -52 * S        # the float64 reference sum's own error (gamma_m in float64): 2^-28 of the bound
        y = y.astype(np.float64)
        worst = np.max((np.abs(y - s) - slack) / np.maximum(gamma * S, 1e-300), initial=0.0, where=m > 0)
        print("operator form: worst |y - s| / (gamma_m S) = %.3g over %d rows" % (worst, shape[0]))
        assert np.all(np.abs(y - s) <= gamma * S + slack)
        assert bits(y[empty]) == bits(np.zeros(int(empty.sum())))
        assert np.all(np.abs(ya.astype(np.float64) - (s + y0.astype(np.float64))) <= gamma1 * (S + np.abs(y0.astype(np.float64))) + slack)
        assert bits(ya[empty]) == bits(y0[empty])


def signed(data, seed):
    rng = np.random.default_rng(seed)
    return (np.asarray(data, dtype=np.float64) * rng.choice([-1.0, 1.0], size=len(data))).astype(np.float32)


def test_rounded_rmat_under_the_small_plans_defaults(hip):
    from sprs_amd import gen
    n = 1 << 14
    ip, ix, dt = gen.rmat_csr(n, 16)
    with band_options(hip):
        check_bound(hip, (n, n), ip.numpy().astype(np.uint64), ix.numpy().astype(np.uint32), signed(dt.numpy(), 71), 72)


@pytest.mark.skipif(EMULATED, reason="a million entries through the fiber emulator: the device run covers it")
def test_rounded_ragged_million(hip):
    rng = np.random.default_rng(53)
    lengths = np.concatenate([rng.integers(0, 5001, size=390), [0, 5000, 1, 0]])
    shape, ip, ix, dt = ragged_csr(lengths, 20000, seed=54, idx=np.uint32, ptr=np.uint64)
    assert 900_000 < ix.size < 1_100_000
    with band_options(hip):
        check_bound(hip, shape, ip, ix, signed(dt, 55), 56)


# ---- contract ----------------------------------------------------------------------------------------------------------------------
def test_plan_selection_contract(hip, long_rows):
    from sprs_amd import _ffi
    from sprs_amd.device import DeviceCsMatF32, DeviceVecF32
    ex = long_rows
    with pytest.raises(_ffi.SprsHipError) as e:
        hip.set_option("spmv_f32_band_tile", 12345)
    assert e.value.status == _ffi.INVALID_ARG
    assert hip.get_option("spmv_f32_band_tile") == 0
    xv = DeviceVecF32.from_host(ex.xs[0])
    # spmv_band = 2 keeps the tile plan; kind is 0 before the first multiply
    hip.set_option("spmv_band", 2)
    try:
        a = DeviceCsMatF32.from_host(ex.shape, ex.ip, ex.ix, ex.dt)
        assert a.spmv_plan_info() == (0, 0)
        y = (a * xv).to_host()
        assert a.spmv_plan_info()[0] == 1 and bits(y) == bits(ex.want[0][0])
    finally:
        hip.set_option("spmv_band", 0)
    # under the automatic rule a small matrix stays on the tile plan, unprepared or prepared, at every multiply
    a = DeviceCsMatF32.from_host(ex.shape, ex.ip, ex.ix, ex.dt)
    for _ in range(3):
        assert bits((a * xv).to_host()) == bits(ex.want[0][0]) and a.spmv_plan_info()[0] == 1
