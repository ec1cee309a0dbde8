"""Single precision on the device: the f32 container, SpMV in both storages, the casts to and from the f64 handle, BiCGSTAB.

Seams of the f32 tile kernel (spmv_f32.hpp), which are those of the f64 one: T = 2048 / 4096 entries per tile (option
spmv_tile); 4 entries per lane and pass on a full tile, the scalar path on the last, partial one; LONG_SEG = 64 (one lane
below, a whole wave from there on); SEG_CHUNK = 2048 row boundaries staged per pass; the carry chain of a row that spans
tiles; tile_of_block's runs of tiles per XCD (tile counts that are no multiple of 8).

Exact cases: integer values and x in [-8, 8], rows of at most 4096 entries (4116 for the one row that has to span three
4096-entry tiles: 4116 * 64 < 2^24 still), so every partial sum is an integer below 2^24 and any summation order gives the
bits of the reference's chain (tests/f32_ref.py).  Rounded cases: the forward-error bound gamma_m * sum |a_k x_k|, which
holds for any order."""
import ctypes as C
import os

import numpy as np
import pytest

import sprs_amd
from sprs_amd import _ffi, gen, linalg, prod
from sprs_amd.device import DeviceCsMat, DeviceCsMatF32, DeviceVec, DeviceVecF32

import f32_ref
from helpers import ragged_csr

pytestmark = pytest.mark.gpu

EMULATED = bool(os.environ.get("SPRS_HIP_LIBRARY"))     # the kernel emulator of tests/emu (tests/test_f32_emu_cpu.py)
CSR, CSC = _ffi.CSR, _ffi.CSC
WIDTHS = [(np.uint32, np.uint32), (np.uint32, np.uint64), (np.uint64, np.uint32), (np.uint64, np.uint64)]   # (indices, indptr)
U = 2.0 ** -24


def bits(a):
    return np.ascontiguousarray(a).tobytes()


@pytest.fixture(params=[2048, 4096])
def tile(request):
    sprs_amd.set_option("spmv_tile", request.param)
    yield request.param
    sprs_amd.set_option("spmv_tile", 0)


# ---- builders -----------------------------------------------------------------------------------------------------
def int_csr(lengths, cols, seed=0, idx=np.uint32, ptr=np.uint32):
    """CSR with the given row lengths, columns c0, c0 + 1, ... (mod cols) per row, integer values in [-8, 8] without 0"""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    assert lengths.max(initial=0) <= cols
    indptr = np.zeros(lengths.size + 1, dtype=np.int64)
    np.cumsum(lengths, out=indptr[1:])
    nnz = int(indptr[-1])
    row_of = np.repeat(np.arange(lengths.size), lengths)
    within = np.arange(nnz) - indptr[row_of]
    start = rng.integers(0, cols, size=lengths.size)
    raw = (start[row_of] + within) % cols
    # sorted inside every row: a wrapped run is rotated so that it ascends
    order = np.lexsort((raw, row_of))
    indices = raw[order]
    vals = rng.integers(1, 9, size=nnz) * rng.choice([-1, 1], size=nnz)
    return (lengths.size, cols), indptr.astype(ptr), indices.astype(idx), vals.astype(np.float32)


def int_vec(n, seed):
    return np.random.default_rng(seed).integers(-8, 9, size=n).astype(np.float32)


def lengths_to(nnz, pattern=(3, 0, 1, 7, 2, 0, 0, 12, 1, 5)):
    out, left, k = [], nnz, 0
    while left:
        n = min(pattern[k % len(pattern)], left)
        out.append(n)
        left -= n
        k += 1
    return out + [0, 0]


def check_exact(m, seed=1):
    """operator and accumulate form against the reference chain, bit for bit; empty rows keep y0 in the accumulate form"""
    shape, ip, ix, dt = m
    a = DeviceCsMatF32.from_host(shape, ip, ix, dt)
    x = int_vec(shape[1], seed)
    y0 = int_vec(shape[0], seed + 1)
    empty = np.flatnonzero(np.diff(ip.astype(np.int64)) == 0)
    if empty.size:
        y0[empty[0]] = np.float32(-0.0)
        y0[empty[-1]] = np.float32(np.nan)
    want = f32_ref.mul_vec(shape, ip, ix, dt, x)
    want_acc = f32_ref.mul_acc_mat_vec_csr(shape, ip, ix, dt, x, y0.copy())
    dx = DeviceVecF32.from_host(x)
    got = (a * dx).to_host()
    assert got.dtype == np.float32 and bits(got) == bits(want)
    assert bits(got[empty]) == bits(np.zeros(empty.size, dtype=np.float32))            # +0.0f
    dy = DeviceVecF32.from_host(y0)
    prod.mul_acc_mat_vec_csr(a, dx, dy)
    got_acc = dy.to_host()
    assert bits(got_acc) == bits(want_acc)
    assert bits(got_acc[empty]) == bits(y0[empty])
    again = (a * dx).to_host()                                                          # the same handle, the same bits
    assert bits(again) == bits(got)
    return a, dx, want


# ---- container ----------------------------------------------------------------------------------------------------
SMALL = int_csr([3, 0, 5, 1, 0, 2, 7], 9, seed=3)


@pytest.mark.parametrize("idx,ptr", WIDTHS)
@pytest.mark.parametrize("storage", [CSR, CSC])
def test_upload_download_round_trip(idx, ptr, storage):
    shape, ip, ix, dt = SMALL
    shape = shape if storage == CSR else shape[::-1]
    dt = dt.copy()
    dt[0], dt[1] = np.float32(-0.0), np.float32(1e-45)       # bits that a value round trip through f64 arithmetic could lose
    a = DeviceCsMatF32.from_host(shape, ip.astype(ptr), ix.astype(idx), dt, storage=storage)
    assert a.shape() == shape and a.nnz() == ix.size and a.storage() == storage
    assert a.index_bytes() == np.dtype(idx).itemsize and a.indptr_bytes() == np.dtype(ptr).itemsize
    s2, ip2, ix2, dt2 = a.to_host()
    assert s2 == shape and ip2.dtype == ptr and ix2.dtype == idx and dt2.dtype == np.float32
    assert np.array_equal(ip2, ip) and np.array_equal(ix2, ix) and bits(dt2) == bits(dt)


def test_upload_rebases_a_sliced_indptr():
    shape, ip, ix, dt = SMALL
    lo = int(ip[2])
    a = DeviceCsMatF32.from_host((shape[0] - 2, shape[1]), ip[2:], ix[lo:], dt[lo:])
    _, ip2, ix2, dt2 = a.to_host()
    assert np.array_equal(ip2, ip[2:] - ip[2]) and np.array_equal(ix2, ix[lo:]) and bits(dt2) == bits(dt[lo:])


def _device_tensors(*arrays):
    """torch tensors on the device (under the kernel emulator, whose device memory IS host memory: CPU tensors)"""
    import torch
    dev = "cpu" if EMULATED else "cuda"
    signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
    return [torch.from_numpy(a.view(signed.get(a.dtype, a.dtype)).copy()).to(dev) for a in arrays]


def test_wrap_device_of_torch_float32_tensors():
    shape, ip, ix, dt = int_csr(lengths_to(700), 40, seed=5, idx=np.uint32, ptr=np.uint64)
    tip, tix, tdt = _device_tensors(ip, ix, dt)
    a = DeviceCsMatF32.wrap_torch(shape, tip, tix, tdt)
    assert a.device_ptrs() == (tip.data_ptr(), tix.data_ptr(), tdt.data_ptr())
    assert a.index_bytes() == 4 and a.indptr_bytes() == 8
    _, ip2, ix2, dt2 = a.to_host()
    assert np.array_equal(ip2, ip) and np.array_equal(ix2, ix) and bits(dt2) == bits(dt)
    x = int_vec(shape[1], 6)
    assert bits((a * DeviceVecF32.from_host(x)).to_host()) == bits(f32_ref.mul_vec(shape, ip, ix, dt, x))
    # values changed in place + refresh: the next product sees them
    tdt.mul_(2.0)
    if not EMULATED:
        import torch
        torch.cuda.synchronize()
    a.refresh()
    assert bits((a * DeviceVecF32.from_host(x)).to_host()) == bits(f32_ref.mul_vec(shape, ip, ix, dt * np.float32(2.0), x))
    with pytest.raises(TypeError):
        DeviceCsMatF32.wrap_torch(shape, tip, tix, tdt.double())


def test_transpose_view_shares_buffers():
    shape, ip, ix, dt = SMALL
    a = DeviceCsMatF32.from_host(shape, ip, ix, dt)
    t = a.transpose_view()
    assert t.device_ptrs() == a.device_ptrs()
    assert t.shape() == shape[::-1] and t.storage() == CSC and t.nnz() == a.nnz()
    assert t.transpose_view().storage() == CSR


def _other_storage_case():
    # one row of the RESULT longer than 1024 entries (column 0 is stored in 1500 rows: the bitmap sort), many result rows
    # of 0, 1 and 2 entries (the wave sort's short cuts) and a few in between
    rng = np.random.default_rng(11)
    rows, cols = 1500, 900
    lengths = rng.integers(1, 4, size=rows)
    ip = np.zeros(rows + 1, dtype=np.int64)
    np.cumsum(lengths, out=ip[1:])
    ix = np.empty(ip[-1], dtype=np.int64)
    for r in range(rows):
        rest = rng.choice(np.arange(1, 300 if r % 3 else cols), size=lengths[r] - 1, replace=False)
        ix[ip[r]:ip[r + 1]] = np.sort(np.concatenate([[0], rest]))
    dt = (np.arange(ix.size) + 1).astype(np.float32) * rng.choice([-1, 1], size=ix.size).astype(np.float32)   # distinct bits
    return (rows, cols), ip, ix, dt


@pytest.mark.parametrize("idx,ptr", [WIDTHS[0], WIDTHS[3]])
def test_to_other_storage_against_the_host_transpose(idx, ptr):
    shape, ip, ix, dt = _other_storage_case()
    _, wp, wi, wd = f32_ref.csc_to_csr(shape[::-1], ip, ix, dt)           # CSR of (r, c) = CSC of the transpose
    counts = np.diff(wp)
    assert counts.max() > 1024 and all(np.count_nonzero(counts == k) > 20 for k in (0, 1, 2))
    a = DeviceCsMatF32.from_host(shape, ip.astype(ptr), ix.astype(idx), dt)
    o = a.to_other_storage()
    assert o.storage() == CSC and o.shape() == shape and o.nnz() == ix.size
    s2, op, oi, od = o.to_host()
    assert op.dtype == ptr and oi.dtype == idx
    assert np.array_equal(op, wp) and np.array_equal(oi, wi) and bits(od) == bits(wd)
    for c in range(shape[1]):
        assert np.all(np.diff(oi[op[c]:op[c + 1]].astype(np.int64)) > 0)
    back = o.to_other_storage()
    _, bp, bi, bd = back.to_host()
    assert back.storage() == CSR and np.array_equal(bp, ip) and np.array_equal(bi, ix) and bits(bd) == bits(dt)


def test_to_f64_then_to_f32_is_the_identity_on_bits():
    shape, ip, ix, dt = int_csr(lengths_to(1000), 50, seed=8)
    dt = dt.copy()
    dt[:6] = np.array([-0.0, 1e-45, np.inf, -np.inf, 3.4028235e38, np.nan], dtype=np.float32)
    a = DeviceCsMatF32.from_host(shape, ip, ix, dt)
    d = a.to_f64()
    assert isinstance(d, DeviceCsMat) and d.index_bytes() == 4 and d.indptr_bytes() == 4
    _, dp, di, dd = d.to_host()
    assert np.array_equal(dp, ip) and np.array_equal(di, ix) and dd.dtype == np.float64
    assert bits(dd[:5]) == bits(dt[:5].astype(np.float64)) and np.isnan(dd[5]) and np.array_equal(dd[6:], dt[6:].astype(np.float64))
    back = d.to_f32()
    assert isinstance(back, DeviceCsMatF32)
    _, bp, bi, bd = back.to_host()
    assert np.array_equal(bp, ip) and np.array_equal(bi, ix) and bits(bd) == bits(dt)


def test_from_f64_rounds_like_a_cast():
    shape, ip, ix, _ = int_csr(lengths_to(600), 50, seed=9, idx=np.uint64, ptr=np.uint64)
    rng = np.random.default_rng(10)
    dt = rng.standard_normal(ix.size) * 10.0 ** rng.integers(-30, 30, size=ix.size)
    dt[:10] = [1e40, -1e40, np.nan, -0.0, 1e-42, 2.0 ** -150, 1.0 + 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50, 3.4028235677973366e38,
               16777217.0]       # inf, -inf, NaN, -0, a denormal result, underflow to 0, a tie (to even), just above it, the overflow edge
    with np.errstate(over="ignore"):
        want = dt.astype(np.float32)
    assert np.isinf(want[0]) and np.isnan(want[2]) and bits(want[3:4]) == bits(np.float32(-0.0)) and 0 < want[4] < 1.2e-38
    a = DeviceCsMat.from_host(shape, ip, ix, dt).to_f32()
    assert a.index_bytes() == 8 and a.indptr_bytes() == 8
    _, ap, ai, ad = a.to_host()
    assert np.array_equal(ap, ip) and np.array_equal(ai, ix)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(ad), nan) and bits(ad[~nan]) == bits(want[~nan])


# ---- SpMV, exact arithmetic ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["1", "3", "4", "5", "T-1", "T", "T+1", "2T+3"])
def test_spmv_exact_entry_counts(tile, which):
    nnz = {"1": 1, "3": 3, "4": 4, "5": 5, "T-1": tile - 1, "T": tile, "T+1": tile + 1, "2T+3": 2 * tile + 3}[which]
    check_exact(int_csr(lengths_to(nnz), 97, seed=nnz))


def test_spmv_exact_one_lane_to_whole_wave(tile):
    check_exact(int_csr([63, 64, 65, 0, 1, 64, 63, 65, 200, 2, 64], 300, seed=21))


def test_spmv_exact_row_across_three_tiles(tile):
    # row 1 starts 10 entries before the end of tile 0, covers tile 1 and ends 10 entries into tile 2
    m = int_csr([tile - 10, tile + 20, 3, 0, 70], tile + 100, seed=22)
    check_exact(m)


def test_spmv_exact_row_ends_on_a_tile_boundary(tile):
    # row 1 crosses the first boundary and ends exactly on the second; row 3 ends exactly on the third; the last row ends the matrix on one
    check_exact(int_csr([tile - 5, tile + 5, 7, tile - 7, tile], tile + 50, seed=23))
    check_exact(int_csr([tile, 9], tile, seed=24))


def test_spmv_exact_more_row_starts_than_one_staged_chunk(tile):
    # runs of empty and one-entry rows: 2 * tile > 2048 row starts inside tile 0 (SEG_CHUNK), then ordinary rows
    check_exact(int_csr([0, 1] * (tile + 300) + [0] * 50 + [5, 64, 0, 3], 200, seed=25))


@pytest.mark.parametrize("ntiles", [9, 17])
def test_spmv_exact_tile_counts_off_the_xcd_multiple(tile, ntiles):
    m = int_csr(lengths_to((ntiles - 1) * tile + 5, pattern=(37, 0, 90, 1, 4096 if tile == 4096 else 1500, 2)), 4200, seed=ntiles)
    a, _, _ = check_exact(m)
    assert (a.nnz() + tile - 1) // tile == ntiles


@pytest.mark.parametrize("idx,ptr", WIDTHS)
def test_spmv_exact_index_widths(tile, idx, ptr):
    check_exact(int_csr(lengths_to(2 * tile + 77, pattern=(3, 0, 70, 1, 640, 0, 9)), 700, seed=31, idx=idx, ptr=ptr))


@pytest.mark.parametrize("idx,ptr", [WIDTHS[0], WIDTHS[3]])
def test_spmv_csc_entries(tile, idx, ptr):
    shape, ip, ix, dt = int_csr(lengths_to(tile + 300, pattern=(3, 0, 70, 1, 200, 0, 9)), 500, seed=41, idx=idx, ptr=ptr)
    _, cp, ci, cd = f32_ref.csc_to_csr(shape[::-1], ip, ix, dt)             # the CSC arrays of the same matrix
    a = DeviceCsMatF32.from_host(shape, cp.astype(ptr), ci.astype(idx), cd, storage=CSC)
    x, y0 = int_vec(shape[1], 42), int_vec(shape[0], 43)
    dx = DeviceVecF32.from_host(x)
    assert bits((a * dx).to_host()) == bits(f32_ref.mul_vec(shape, ip, ix, dt, x))
    dy = DeviceVecF32.from_host(y0)
    prod.mul_acc_mat_vec_csc(a, dx, dy)
    assert bits(dy.to_host()) == bits(f32_ref.mul_acc_mat_vec_csr(shape, ip, ix, dt, x, y0.copy()))
    assert bits((a * dx).to_host()) == bits(f32_ref.mul_vec(shape, ip, ix, dt, x))      # the cached CSR form again
    # an all-empty matrix: the operator form writes +0.0, the accumulate form nothing
    z = DeviceCsMatF32.from_host((3, 4), np.zeros(4, dtype=ptr), np.zeros(0, dtype=idx), np.zeros(0, dtype=np.float32))
    x4, y3 = DeviceVecF32.from_host(int_vec(4, 1)), DeviceVecF32.from_host(np.array([1, -0.0, 2], dtype=np.float32))
    assert bits((z * x4).to_host()) == bits(np.zeros(3, dtype=np.float32))
    prod.mul_acc_mat_vec_csr(z, x4, y3)
    assert bits(y3.to_host()) == bits(np.array([1, -0.0, 2], dtype=np.float32))


# ---- SpMV, rounded arithmetic ----------------------------------------------------------------------------------------
def _check_bound(shape, ip, ix, dt, seed):
    """|y_i - s_i| <= gamma_m S_i (operator form) and gamma_{m+1} (S_i + |y0_i|) (accumulate form), every row"""
    rng = np.random.default_rng(seed)
    ip64 = ip.astype(np.int64)
    m = np.diff(ip64).astype(np.float64)
    x = ((rng.random(shape[1]) + 0.5) * rng.choice([-1.0, 1.0], size=shape[1])).astype(np.float32)
    y0 = ((rng.random(shape[0]) + 0.5) * rng.choice([-1.0, 1.0], size=shape[0])).astype(np.float32)
    p = dt.astype(np.float64) * x.astype(np.float64)[ix.astype(np.int64)]
    # per-row sums in float64 (reduceat on a padded array: an empty row reads one element, zeroed below)
    S = np.where(m > 0, np.add.reduceat(np.concatenate([np.abs(p), [0.0]]), ip64[:-1]), 0.0)
    s = np.where(m > 0, np.add.reduceat(np.concatenate([p, [0.0]]), ip64[:-1]), 0.0)
    slack = m * 2.0 ** -52 * S        # the float64 reference sum's own error (gamma_m in float64): 2^-28 of the bound
    a = DeviceCsMatF32.from_host(shape, ip, ix, dt)
    dx = DeviceVecF32.from_host(x)
    y = (a * dx).to_host().astype(np.float64)
    gamma = m * U / (1.0 - m * U)
    worst = np.max((np.abs(y - s) - slack) / np.maximum(gamma * S, 1e-300), initial=0.0, where=m > 0)
    print("operator form: worst |y - s| / (gamma_m S) = %.3g over %d rows" % (worst, shape[0]))
    assert np.all(np.abs(y - s) <= gamma * S + slack)
    empty = m == 0
    assert bits(y[empty]) == bits(np.zeros(int(empty.sum())))
    dy = DeviceVecF32.from_host(y0)
    prod.mul_acc_mat_vec_csr(a, dx, dy)
    ya = dy.to_host()
    gamma1 = (m + 1) * U / (1.0 - (m + 1) * U)
    assert np.all(np.abs(ya.astype(np.float64) - (s + y0.astype(np.float64))) <= gamma1 * (S + np.abs(y0.astype(np.float64))) + slack)
    assert bits(ya[empty]) == bits(y0[empty])


def _signed(data, seed):
    rng = np.random.default_rng(seed)
    return (np.asarray(data, dtype=np.float64) * rng.choice([-1.0, 1.0], size=len(data))).astype(np.float32)


def test_spmv_rounded_rmat():
    n = 60000
    ip, ix, dt = gen.rmat_csr(n, 16)
    ip, ix = ip.numpy().astype(np.uint64), ix.numpy().astype(np.uint32)
    _check_bound((n, n), ip, ix, _signed(dt.numpy(), 51), 52)


def test_spmv_rounded_ragged_million():
    rng = np.random.default_rng(53)
    lengths = np.concatenate([rng.integers(0, 5001, size=390), [0, 5000, 1, 0]])
    shape, ip, ix, dt = ragged_csr(lengths, 20000, seed=54, idx=np.uint32, ptr=np.uint64)
    assert 900_000 < ix.size < 1_100_000
    _check_bound(shape, ip, ix, _signed(dt, 55), 56)


# ---- BiCGSTAB ----------------------------------------------------------------------------------------------------------
def _solve(a, x0, b, tol, max_iter):
    return linalg.BiCGSTAB.solve(a, DeviceVecF32.from_host(x0), DeviceVecF32.from_host(b), tol, max_iter)


def test_bicgstab_reference_f32_system_bit_for_bit():
    csc = f32_ref.REF_SYSTEM_CSC
    csr = f32_ref.csc_to_csr(*csc)
    one = np.ones(4, dtype=np.float32)
    want, ok = f32_ref.BiCGSTAB.solve(csr, one, one, f32_ref.REF_TOL, f32_ref.REF_MAX_ITER)
    assert ok
    results = []
    for m, storage in ((csc, CSC), (csr, CSR)):
        a = DeviceCsMatF32.from_host(m[0], m[1].astype(np.uint64), m[2].astype(np.uint64), m[3], storage=storage)
        res = _solve(a, one, one, f32_ref.REF_TOL, f32_ref.REF_MAX_ITER)
        x = res.x().to_host()
        assert res.converged and x.dtype == np.float32 and bits(x) == bits(want.x)
        assert (res.iteration_count(), res.soft_restart_count(), res.hard_restart_count()) == (
            want.iteration_count, want.soft_restart_count, want.hard_restart_count)
        assert bits(np.float32(res.err())) == bits(want.err) and float(np.float32(res.err())) == res.err()      # widened exactly
        assert bits(np.float32(res.rho())) == bits(want.rho) and float(np.float32(res.rho())) == res.rho()
        results.append(bits(x))
        # the reference's own assertion
        b_rec = f32_ref.mul_vec(*csr, x)
        assert np.all(np.abs(np.float32(1.0) - one / b_rec) < np.float32(f32_ref.REF_TOL))
    assert results[0] == results[1]                      # a CSC operand gives the bits of its CSR form


def _tridiagonal(n):
    ip = np.zeros(n + 1, dtype=np.int64)
    ip[1:] = np.cumsum(np.where((np.arange(n) == 0) | (np.arange(n) == n - 1), 2, 3))
    ix = np.concatenate([[c for c in (r - 1, r, r + 1) if 0 <= c < n] for r in range(n)]).astype(np.uint32)
    dt = np.where(ix == np.repeat(np.arange(n), np.diff(ip)), 4.0, -1.0).astype(np.float32)
    return (n, n), ip.astype(np.uint32), ix, dt


def test_bicgstab_tree_dots_converge_and_the_true_residual_is_below_tol():
    n, tol = 3000, 1e-4                                   # n > 2048: the two-level tree dots
    m = _tridiagonal(n)
    rng = np.random.default_rng(61)
    b = ((rng.random(n) + 0.5) / 64.0).astype(np.float32)
    x0 = np.zeros(n, dtype=np.float32)
    res = _solve(DeviceCsMatF32.from_host(*m), x0, b, tol, 200)
    assert res.converged and 0 < res.iteration_count() < 200 and res.hard_restart_count() >= 1
    x = res.x().to_host()
    r = b - f32_ref.mul_vec(*m, x)                        # the true residual, recomputed in f32 on the host
    err = float(np.sqrt(np.sum(r.astype(np.float64) ** 2)))
    print("n = %d: %d iterations, device err %.3g, host residual %.3g" % (n, res.iteration_count(), res.err(), err))
    assert err < tol and res.err() < tol
    # a CSC operand gives the same bits
    _, cp, ci, cd = f32_ref.csc_to_csr(m[0], m[1], m[2], m[3])
    res_c = _solve(DeviceCsMatF32.from_host(m[0], cp.astype(np.uint32), ci.astype(np.uint32), cd, storage=CSC), x0, b, tol, 200)
    assert bits(res_c.x().to_host()) == bits(x) and res_c.iteration_count() == res.iteration_count()
    # too few iterations: Err(solver), results still inside
    short = _solve(DeviceCsMatF32.from_host(*m), x0, b, 1e-30, 2)
    assert not short.converged and short.iteration_count() == 2 and short.err() > 0


# ---- errors ----------------------------------------------------------------------------------------------------------------
def test_contract_violations():
    shape, ip, ix, dt = SMALL
    a = DeviceCsMatF32.from_host(shape, ip, ix, dt)
    c = a.to_other_storage()
    x, y = DeviceVecF32.zeros(shape[1]), DeviceVecF32.zeros(shape[0])
    with pytest.raises(_ffi.SprsHipError) as e:
        prod.mul_acc_mat_vec_csr(c, x, y)
    assert e.value.status == _ffi.STORAGE_MISMATCH and "Storage mismatch" in str(e.value)
    with pytest.raises(_ffi.SprsHipError) as e:
        prod.mul_acc_mat_vec_csc(a, x, y)
    assert e.value.status == _ffi.STORAGE_MISMATCH
    for mat in (a, c):
        with pytest.raises(_ffi.SprsHipError) as e:
            prod.csmat_mul_vec(mat, y, out=x)
        assert e.value.status == _ffi.DIM_MISMATCH and "Dimension mismatch" in str(e.value)
    with pytest.raises(_ffi.SprsHipError) as e:       # dimensions are tested before the storage (prod.rs:114-118)
        prod.mul_acc_mat_vec_csr(c, y, x)
    assert e.value.status == _ffi.DIM_MISMATCH
    with pytest.raises(_ffi.SprsHipError) as e:
        linalg.BiCGSTAB.solve(a, x, x, 1e-6, 5)       # not square
    assert e.value.status == _ffi.DIM_MISMATCH
    with pytest.raises(_ffi.SprsHipError) as e:
        DeviceCsMatF32.from_host(shape, ip.astype(np.uint16), ix.astype(np.uint16), dt)
    assert e.value.status == _ffi.INVALID_ARG and "2-byte" in str(e.value)
    with pytest.raises(_ffi.SprsHipError) as e:
        DeviceCsMatF32.from_host(shape, ip, ix[::-1].copy(), dt)
    assert e.value.status == _ffi.BAD_STRUCTURE
    # one precision per product
    d = a.to_f64()
    with pytest.raises(TypeError):
        a * DeviceVec.zeros(shape[1])
    with pytest.raises(TypeError):
        d * x
    with pytest.raises(TypeError):
        prod.mul_acc_mat_vec_csr(d, x, y)
    with pytest.raises(TypeError):
        prod.mul_acc_mat_vec_csr(a, DeviceVec.zeros(shape[1]), y)


def test_device_vec_f32_borrow_needs_four_byte_elements():
    t64, t32 = _device_tensors(np.zeros(4), np.arange(4, dtype=np.float32))
    with pytest.raises(TypeError):
        DeviceVecF32.borrow(t64)
    if not EMULATED:
        v = DeviceVecF32.borrow(t32)
        assert v.n == 4 and v.ptr == t32.data_ptr() and bits(v.to_host()) == bits(np.arange(4, dtype=np.float32))
    with np.errstate(over="ignore"):
        assert DeviceVecF32.from_host(np.array([1.0 + 2.0 ** -24, 1e40])).to_host().tolist() == [1.0, np.inf]    # casts to float32


def test_spmv_on_a_capturing_stream_needs_the_plan():
    """an SpMV captured into a graph: INVALID_ARG without the plan; with it the call is captured and replays to the same bits"""
    import torch
    shape, ip, ix, dt = int_csr(lengths_to(3 * 2048 + 11, pattern=(3, 0, 70, 1, 2300, 0, 9)), 2400, seed=71)
    x = int_vec(shape[1], 72)
    want = f32_ref.mul_vec(shape, ip, ix, dt, x)
    a, fresh = DeviceCsMatF32.from_host(shape, ip, ix, dt), DeviceCsMatF32.from_host(shape, ip, ix, dt)
    tx = torch.from_numpy(x).cuda()
    ty = torch.full((shape[0],), 7.0, dtype=torch.float32, device="cuda")
    dx, dy = DeviceVecF32.borrow(tx), DeviceVecF32.borrow(ty)
    s = torch.cuda.Stream()
    a.prepare(stream=s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    sp = C.c_void_p(s.cuda_stream)
    with torch.cuda.graph(g, stream=s):
        st_fresh = _ffi.lib.sprs_hip_spmv_f32(fresh._h, C.c_void_p(dx.ptr), dx.n, C.c_void_p(dy.ptr), dy.n, 0, sp)
        msg = _ffi.lib.sprs_hip_last_error()
        st = _ffi.lib.sprs_hip_spmv_f32(a._h, C.c_void_p(dx.ptr), dx.n, C.c_void_p(dy.ptr), dy.n, 0, sp)
    assert st_fresh == _ffi.INVALID_ARG and b"sprs_hip_csmat_f32_prepare" in msg
    assert st == _ffi.OK
    torch.cuda.synchronize()
    assert bits(ty.cpu().numpy()) == bits(np.full(shape[0], 7.0, dtype=np.float32))      # captured, not run
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert bits(ty.cpu().numpy()) == bits(want)
        ty.fill_(7.0)
    torch.cuda.synchronize()
    assert bits((a * dx).to_host()) == bits(want)                                          # and eagerly, the same bits
