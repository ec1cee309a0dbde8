"""PACKED hot slices of the banded SpMV plan (sprs_amd/csrc/spmv_band_kernels.hpp, "PACKED hot slices"; option spmv_band_pack):
a hot slice whose wave tiles of 512 entries hold at most two sign / exponent patterns ("keys") each is stored at 8.5 instead of
10 bytes per entry.  The packing is lossless and leaves the order of the additions alone, so the criterion everywhere is BIT
EQUALITY of y between spmv_band_pack = 1 and = 2 (compared as uint64), for the operator and the accumulate form and run to run;
parity with the CPU oracle (<= 1e-10 relative, the bar of test_spmv_band_gpu.py) comes on top.

Which slices were packed is read off plan_bytes.  With T hot tiles of which P are packed, the raw plan holds (512 T + 512) x 10
bytes of hot entries; a plan whose slices are all packed holds 4352 T, one with raw slices left (512 (T - P) + 512) x 10 + 4352 P:
    raw - packed = 768 T + 5120   (every slice packed: 1.5 bytes per entry of the padded tiles, and the raw arrays' spare tile)
    raw - packed = 768 P - 64 W   (some slices left raw; W hot workgroups whose share holds slices of both forms are cut in two,
                                   one 64-byte record each)
and 5120 = 512 mod 768 tells the first form from the second as long as W is 0, i.e. always when every slice is packed.

The same file runs through the kernel emulator on the CPU (tests/test_band_pack_emu_cpu.py)."""
import os

import numpy as np
import pytest

from conftest import IDX_COMBOS
from helpers import ragged_csr, rel_err

pytestmark = pytest.mark.gpu

EMULATED = bool(os.environ.get("SPRS_HIP_LIBRARY"))     # the kernel emulator of tests/emu: its device memory is host memory
TOL = 1e-10
REC_SAVED = 768          # bytes a packed tile saves: 512 x 1.5
SPARE = 5120             # the raw arrays' spare tile: 512 x 10


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


def oracle_spmv(shape, ip, ix, dt, x, y=None):
    from oracle import oracle
    out = np.zeros(shape[0]) if y is None else y.copy()
    oracle.mul_acc_mat_vec_csr(shape, ip.astype(np.uint64), ix.astype(np.uint64), dt, x, out)
    return out


def u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def run_plan(hip, shape, ip, ix, dt, x, y0, pack, **opts):
    """-> (y = A x, y0 + A x, plan bytes) under spmv_band_pack = pack; every product is taken twice (run-to-run determinism)"""
    from sprs_amd import prod
    from sprs_amd.device import DeviceCsMat, DeviceVec
    with band_options(hip, spmv_band_pack=pack, **opts):
        a = DeviceCsMat.from_host(shape, ip, ix, dt)
        xv = DeviceVec.from_host(x)
        y = (a * xv).to_host()
        kind, nbytes = a.spmv_plan_info()
        assert kind == 3                                       # (a case that falls back to another plan tests nothing)
        assert np.array_equal(u64(y), u64((a * xv).to_host()))
        acc = []
        for _ in range(2):
            yv = DeviceVec.from_host(y0)
            prod.mul_acc_mat_vec_csr(a, xv, yv)
            acc.append(yv.to_host())
        assert np.array_equal(u64(acc[0]), u64(acc[1]))
        assert a.spmv_plan_info() == (kind, nbytes)
    return y, acc[0], nbytes


def check_pack(hip, shape, ip, ix, dt, seed=0, x=None, oracle_exact=False, **opts):
    """both forms of the product, packed against raw bit for bit, and against the oracle; -> raw bytes - packed bytes"""
    rng = np.random.default_rng(seed)
    if x is None:
        x = rng.random(shape[1]) + 0.5
    y0 = rng.integers(1, 9, size=shape[0]).astype(np.float64)
    y1, acc1, b1 = run_plan(hip, shape, ip, ix, dt, x, y0, 1, **opts)
    y2, acc2, b2 = run_plan(hip, shape, ip, ix, dt, x, y0, 2, **opts)
    nan = np.isnan(y2)
    assert np.array_equal(np.isnan(y1), nan) and np.array_equal(np.isnan(acc1), np.isnan(acc2))
    assert np.array_equal(u64(y1)[~nan], u64(y2)[~nan])
    assert np.array_equal(u64(acc1)[~np.isnan(acc2)], u64(acc2)[~np.isnan(acc2)])
    ref, ref_acc = oracle_spmv(shape, ip, ix, dt, x), oracle_spmv(shape, ip, ix, dt, x, y=y0)
    assert np.array_equal(np.isnan(ref), nan)
    if oracle_exact:
        assert np.array_equal(u64(y1)[~nan], u64(ref)[~nan]) and np.array_equal(u64(acc1)[~nan], u64(ref_acc)[~nan])
    else:
        fin = np.isfinite(ref)
        assert np.array_equal(y1[~fin & ~nan], ref[~fin & ~nan])
        assert rel_err(y1[fin], ref[fin]) <= TOL and rel_err(acc1[fin], ref_acc[fin]) <= TOL
    empty = np.diff(ip.astype(np.int64)) == 0
    assert np.all(y1[empty] == 0.0) and np.array_equal(acc1[empty], y0[empty])
    return b2 - b1


def all_packed_tiles(diff):
    """the number of hot tiles of a plan whose slices were ALL packed (asserted), from raw bytes - packed bytes"""
    assert diff > 0 and diff % REC_SAVED == SPARE % REC_SAVED, "hot slices were left raw (bytes saved: %d)" % diff
    return (diff - SPARE) // REC_SAVED


def long_rows_matrix(rows=260, cols=20000, seed=0, idx=np.uint64, ptr=np.uint64):
    """long rows of 40 .. 200 entries (split 2: their entries are all hot when the slices cover every column) between empty rows
    and rows of one entry (short) -> shape, indptr, indices, data in [0.5, 1.5), hot entries"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(40, 200, size=rows)
    lens[::9] = 0
    lens[4::11] = 1
    shape, ip, ix, dt = ragged_csr([int(v) for v in lens], cols, seed=seed, idx=idx, ptr=ptr)
    return shape, ip, ix, dt, int(lens[lens >= 2].sum())


# 20 000 columns: three slices of 8192 labels or two of 16384 cover them
TILES = [(8192, 3), (16384, 2)]


@pytest.mark.parametrize("tile,hot", TILES)
@pytest.mark.parametrize("idx,ptr", IDX_COMBOS)
def test_values_of_one_magnitude_class_pack_every_slice(hip, idx, ptr, tile, hot):
    """cases 1, 6, 7: every value in [0.5, 1.5) (two keys): every slice packs, and the plan shrinks by exactly 1.5 bytes per hot
    entry of the padded tiles — at least ceil(entries / 512) tiles, at most one partly filled tile per slice more"""
    shape, ip, ix, dt, hot_nnz = long_rows_matrix(idx=idx, ptr=ptr)
    assert dt.min() >= 0.5 and dt.max() < 1.5 and (dt < 1.0).any() and (dt >= 1.0).any()
    diff = check_pack(hip, shape, ip, ix, dt, spmv_band_tile=tile, spmv_band_hot=hot, spmv_band_split=2)
    tiles = all_packed_tiles(diff)
    assert -(-hot_nnz // 512) <= tiles <= hot_nnz // 512 + hot


def test_a_tile_with_three_keys_keeps_its_slice_raw(hip):
    """case 2: two columns that every long row references (the two most popular: labels 0 and 1, in slice 0) carry 2.0 and 4.0
    beside values in [0.5, 1.5): every tile of slice 0 holds four keys, so slice 0 stays raw and the other slices pack.  With those
    two columns' values back in [0.5, 1.5) the same structure packs whole."""
    rng = np.random.default_rng(5)
    rows, cols = 400, 20000
    shape, ip, ix, dt = ragged_csr([60] * rows, cols - 2, seed=5)
    ix = ix + 2                                                 # columns 0 and 1 are free: every row takes them
    lens = np.full(rows, 62)
    ip2 = np.zeros(rows + 1, dtype=np.uint64)
    ip2[1:] = np.cumsum(lens)
    ix2 = np.concatenate([np.concatenate([[0, 1], ix[int(ip[r]):int(ip[r + 1])]]) for r in range(rows)]).astype(np.uint64)
    dt2 = rng.random(ix2.size) + 0.5
    hubs = np.flatnonzero(ix2 < 2)
    plain = dt2.copy()
    dt2[hubs] = np.where(ix2[hubs] == 0, 2.0, 4.0)
    opts = dict(spmv_band_tile=8192, spmv_band_hot=3, spmv_band_split=2)
    whole = all_packed_tiles(check_pack(hip, (rows, cols), ip2, ix2, plain, seed=1, **opts))
    diff = check_pack(hip, (rows, cols), ip2, ix2, dt2, seed=1, **opts)
    # some slices packed, slice 0 left raw: it holds at least the 2 x rows entries of the two columns
    assert 0 < diff <= REC_SAVED * (whole - -(-2 * rows // 512))


@pytest.mark.parametrize("n", [1, 511, 512, 513, 1025])
def test_slice_sizes_at_the_record_seams(hip, n):
    """case 3: 8192 + n columns referenced once each (one popularity class: labels in column order), so slice 0 holds 8192 entries
    = 16 tiles and slice 1 exactly n: one entry, a tile short of one, a whole tile, one entry more, two tiles and one entry"""
    total = 8192 + n
    lens = [64] * (total // 64 - 1) + [64 + total % 64]
    ip = np.zeros(len(lens) + 1, dtype=np.uint64)
    ip[1:] = np.cumsum(lens)
    ix = (3 * np.arange(total)).astype(np.uint64)
    rng = np.random.default_rng(n)
    dt = rng.random(total) + 0.5
    diff = check_pack(hip, (len(lens), 3 * total), ip, ix, dt, seed=n, spmv_band_tile=8192, spmv_band_hot=2, spmv_band_split=2, spmv_band_hot_run=1)
    assert all_packed_tiles(diff) == 16 + -(-n // 512)


def test_hub_rows_over_many_segments(hip):
    """three dense rows (every slice sees rows that span several tiles, ranges and workgroups: register carries, head carries, runs of
    ranges without a row start) between rows of 33 entries, under one to forty hot workgroups per CU and ranges of one tile up to a
    whole segment: the packed records are found through the segment's first record wherever a segment starts in a slice"""
    lens = [0, 20000, 3, 0] + [33] * 700 + [20000] + [1, 0, 31, 32] * 20 + [33] * 700 + [20000, 0, 0, 7]
    shape, ip, ix, dt = ragged_csr(lens, 20000, seed=3)
    for rounds, tile, hot, run in ((1, 8192, 2, 0), (3, 16384, 2, 1), (40, 8192, 3, 3), (2, 16384, 1, 1000)):
        diff = check_pack(hip, shape, ip, ix, dt, seed=rounds, spmv_band_tile=tile, spmv_band_hot=hot, spmv_band_rounds=rounds,
                          spmv_band_hot_run=run, spmv_band_phases=2)
        assert all_packed_tiles(diff) > 0


def test_two_ranges_per_wave_and_turn(hip):
    """a BIG plan's packed slices are walked two consecutive ranges per wave and turn (HotSeg::group).  Big means at least 400 hot
    tiles per CU: the emulator's chip of 4 CUs reaches that with these 1 611 tiles (on the device the same matrix is a small plan
    and runs as the other cases do).  Rows of 3 300 entries cross tiles, ranges, groups and workgroups; which wave walks a range
    must not change a bit of y"""
    shape, ip, ix, dt = ragged_csr([3300, 0, 5, 3300] * 125, 20000, seed=11)
    diff = check_pack(hip, shape, ip, ix, dt, seed=11, spmv_band_tile=8192, spmv_band_hot=3, spmv_band_split=8)
    assert all_packed_tiles(diff) >= 2 * 125 * 3300 // 512 >= 400 * 4


@pytest.mark.parametrize("tile,hot", TILES)
def test_keys_that_differ_in_sign_only(hip, tile, hot):
    """case 4: values +-[1, 2): the two keys of a tile differ in the sign bit alone"""
    shape, ip, ix, dt, hot_nnz = long_rows_matrix(seed=4)
    rng = np.random.default_rng(4)
    dt = np.where(rng.random(dt.size) < 0.5, -1.0, 1.0) * (1.0 + rng.random(dt.size))
    dt[::3] = np.where(dt[::3] < 0, -1.0, 1.0)                  # +-1.0 itself
    diff = check_pack(hip, shape, ip, ix, dt, seed=4, spmv_band_tile=tile, spmv_band_hot=hot, spmv_band_split=2)
    assert all_packed_tiles(diff) >= -(-hot_nnz // 512)


def test_zeros_and_denormals(hip):
    """case 5: +-0.0 and denormals down to the smallest (keys 0x000 and 0x800).  x holds integers 1 .. 4: every product and every
    sum is a multiple of 2^-1074 below 200 x 4 x 1e-311 < 2^-1021, hence exact in any order — the oracle's bits are the only
    right answer"""
    shape, ip, ix, dt, hot_nnz = long_rows_matrix(seed=6)
    rng = np.random.default_rng(6)
    pool = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-311, -3e-320, 7e-312])
    dt = pool[rng.integers(0, pool.size, size=dt.size)]
    x = rng.integers(1, 5, size=shape[1]).astype(np.float64)
    diff = check_pack(hip, shape, ip, ix, dt, seed=6, x=x, oracle_exact=True, spmv_band_tile=8192, spmv_band_hot=3, spmv_band_split=2)
    assert all_packed_tiles(diff) >= -(-hot_nnz // 512)


def test_infinities_and_nans_with_payload(hip):
    """case 5: +Inf and NaNs with payloads (key 0x7ff, any mantissa) in a few rows beside values in [1, 2): identical NaN masks,
    and the bits of every other result equal"""
    shape, ip, ix, dt, hot_nnz = long_rows_matrix(seed=7)
    rng = np.random.default_rng(7)
    dt = 1.0 + rng.random(dt.size)
    special = np.array([0x7FF0000000000000, 0x7FF0000000000001, 0x7FF8DEADBEEF0123, 0x7FFFFFFFFFFFFFFF], dtype=np.uint64).view(np.float64)
    long_rows = np.flatnonzero(np.diff(ip.astype(np.int64)) >= 2)
    for j, r in enumerate(long_rows[[0, 3, 50, 51, 120]]):
        lo, hi = int(ip[r]), int(ip[r + 1])
        dt[lo + j:hi:7] = special[j % special.size]
    diff = check_pack(hip, shape, ip, ix, dt, seed=7, spmv_band_tile=8192, spmv_band_hot=3, spmv_band_split=2)
    assert all_packed_tiles(diff) >= -(-hot_nnz // 512)


def test_generator_values_pack_every_slice(hip):
    """the reference generator's values (U[0.5, 1.5)) leave NO hot slice raw: gen.rmat_csr(1 << 14, 16) under the default slices
    and split of a small plan"""
    from sprs_amd import gen
    n = 1 << 14
    indptr, indices, data = gen.rmat_csr(n, 16)
    ip, ix, dt = indptr.numpy().astype(np.uint64), indices.numpy().astype(np.uint64), data.numpy()
    diff = check_pack(hip, (n, n), ip, ix, dt, seed=8)
    assert all_packed_tiles(diff) > 0


def test_value_update_in_place_packs_again(hip):
    """case 8: the handle wraps device arrays; values changed in place + refresh() build the plan, and with it the packed copy,
    again: doubled values (still two keys) pack again, a third key in every tile falls back to the raw arrays — same bits as a
    fresh raw plan each time"""
    import torch
    from sprs_amd.device import DeviceCsMat, DeviceVec
    shape, ip, ix, dt, hot_nnz = long_rows_matrix(seed=9)
    dev = "cpu" if EMULATED else "cuda"
    tip, tix, tdt = [torch.from_numpy(a.view(np.int64).copy() if a.dtype == np.uint64 else a.copy()).to(dev) for a in (ip, ix, dt)]
    x = np.random.default_rng(9).random(shape[1]) + 0.5
    opts = dict(spmv_band_tile=8192, spmv_band_hot=3, spmv_band_split=2)

    def raw_plan(values):
        with band_options(hip, spmv_band_pack=2, **opts):
            a = DeviceCsMat.from_host(shape, ip, ix, values)
            y = (a * DeviceVec.from_host(x)).to_host()
            return y, a.spmv_plan_info()[1]

    def sync():
        if not EMULATED:
            torch.cuda.synchronize()

    with band_options(hip, spmv_band_pack=1, **opts):
        a = DeviceCsMat.wrap_torch(shape, tip, tix, tdt)
        xv = DeviceVec.from_host(x)
        y = (a * xv).to_host()
        nbytes = a.spmv_plan_info()[1]
    y_raw, raw_bytes = raw_plan(dt)
    assert np.array_equal(u64(y), u64(y_raw))
    tiles = all_packed_tiles(raw_bytes - nbytes)

    tdt.mul_(2.0)                                               # [1, 3): keys 0x3ff and 0x400
    sync()
    with band_options(hip, spmv_band_pack=1, **opts):
        a.refresh()
        y = (a * xv).to_host()
        assert a.spmv_plan_info() == (3, nbytes)
    assert np.array_equal(u64(y), u64(raw_plan(2.0 * dt)[0]))
    assert all_packed_tiles(raw_bytes - nbytes) == tiles

    tdt[::5] = 8.0                                              # a third key (0x402) in every tile
    sync()
    dt3 = 2.0 * dt
    dt3[::5] = 8.0
    with band_options(hip, spmv_band_pack=1, **opts):
        a.refresh()
        y = (a * xv).to_host()
        assert a.spmv_plan_info() == (3, raw_bytes)             # every slice raw again
    assert np.array_equal(u64(y), u64(raw_plan(dt3)[0]))
