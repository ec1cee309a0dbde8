"""f32 SpMM on the device: `&CsMat<f32> * &Array2<f32>`, the four mulacc_dense forms, `Array2::dot(&CsMat)`.

Constants of the shipped kernel (spmm_f32.hpp / spmm.hip): tile T = 256 entries per wave, four waves per workgroup; column
blocks of 64; column-group classes of 8 / 16 / 32 / 64 columns — scalar lanes: groups of 8 / 16 / 32 / 64 lanes, paired lanes
(option spmm_f32_pair = 2; 1 = auto takes them for the 32- and 64-column classes under >= 8 entries per row; two columns per
lane): groups of 4 / 8 / 16 / 32 lanes; FIX_SPAN = 8 tiles for the short fix-up; the
re-laid-out rhs in blocks of 4096 rows; the hypersparse rule rows > 4 nnz + 4096; chunks of 512 entries under spmm_stream = 0.
K_CLASSES below are every class, each block seam at -1 / 0 / +1, and odd k.

Exact cases: values, rhs and the initial result are integers in [-8, 8], rows have at most 4096 entries, so every partial sum is
an integer below 2^24 and ANY summation order gives the bits of the reference's chain (tests/spmm_f32_ref.py).  Every caller
buffer lies between NaN guard words and has NaN words in its padding; they must come back untouched.  Rounded cases: the
forward-error bound gamma_m * sum |a b|, which holds for any order."""
import ctypes as C
import os

import numpy as np
import pytest

import sprs_amd
from sprs_amd import _ffi, gen, prod
from sprs_amd.device import DeviceCsMat, DeviceCsMatF32, DeviceVec, DeviceVecF32

import f32_ref
import spmm_f32_ref
from helpers import ragged_csr

pytestmark = pytest.mark.gpu

EMULATED = bool(os.environ.get("SPRS_HIP_LIBRARY"))     # the kernel emulator of tests/emu (tests/test_spmm_f32_emu_cpu.py)
CSR, CSC, ROW, COL = _ffi.CSR, _ffi.CSC, _ffi.ROW_MAJOR, _ffi.COL_MAJOR
WIDTHS = [(np.uint32, np.uint32), (np.uint32, np.uint64), (np.uint64, np.uint32), (np.uint64, np.uint64)]   # (indices, indptr)
U = 2.0 ** -24
T, FIX_SPAN, CHUNK = 256, 8, 512
K_CLASSES = [1, 2, 7, 8, 9, 15, 16, 17, 24, 31, 32, 33, 63, 64, 65, 129]
GUARD_BITS = np.uint32(0x7FC0BEEF)                      # a quiet NaN with a payload no computation produces
# (name, spmm_long_row, spmm_stream, spmm_relayout)
MODES = (("stream", 0, 1, 2), ("stream-relaid-rhs", 0, 1, 1), ("chunks", 0, 0, 2), ("entry-order", 2048, 1, 2))


def bits(a):
    return np.ascontiguousarray(a).tobytes()


@pytest.fixture(params=[2, 1, 0], ids=["paired", "auto", "scalar"])
def pair(request):
    sprs_amd.set_option("spmm_f32_pair", request.param)
    yield request.param
    sprs_amd.set_option("spmm_f32_pair", 1)


@pytest.fixture(params=MODES, ids=[m[0] for m in MODES])
def mode(request):
    _, long_row, stream, relayout = request.param
    sprs_amd.set_option("spmm_long_row", long_row)
    sprs_amd.set_option("spmm_stream", stream)
    sprs_amd.set_option("spmm_relayout", relayout)
    yield request.param[0]
    sprs_amd.set_option("spmm_long_row", -1)
    sprs_amd.set_option("spmm_stream", 1)
    sprs_amd.set_option("spmm_relayout", 0)


# ---- builders -----------------------------------------------------------------------------------------------------
def int_csr(lengths, cols, seed=0, idx=np.uint32, ptr=np.uint32):
    """CSR with the given row lengths, a run of consecutive columns (mod cols) per row, integer values in [-8, 8] without 0"""
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
    indices = raw[np.lexsort((raw, row_of))]
    vals = rng.integers(1, 9, size=nnz) * rng.choice([-1, 1], size=nnz)
    return (lengths.size, cols), indptr.astype(ptr), indices.astype(idx), vals.astype(np.float32)


def int_mat(shape, seed):
    return np.random.default_rng(seed).integers(-8, 9, size=shape).astype(np.float32)


def lengths_to(nnz, pattern=(3, 0, 1, 7, 2, 0, 0, 12, 1, 5)):
    out, left, k = [], nnz, 0
    while left:
        n = min(pattern[k % len(pattern)], left)
        out.append(n)
        left -= n
        k += 1
    return out + [0, 0]


class Guarded:
    """a caller's dense buffer on the device: `lead` guard words, lines of `ld` floats (the matrix in the first `width` of each,
    guard words in the padding), 8 guard words.  lead = 8 leaves the matrix 8-byte aligned, an odd lead does not."""

    def __init__(self, arr, col_major=False, ld=None, lead=8):
        arr = np.asarray(arr, dtype=np.float32)
        self.shape, self.col_major, self.lead = arr.shape, col_major, lead
        lines = arr.T if col_major else arr
        self.nl, self.w = lines.shape
        self.ld = self.w if ld is None else int(ld)
        assert self.ld >= self.w
        img = np.full(lead + self.nl * self.ld + 8, GUARD_BITS, dtype=np.uint32).view(np.float32)
        if self.nl and self.w:
            img[lead:lead + self.nl * self.ld].reshape(self.nl, self.ld)[:, :self.w] = lines
        self.img = img
        self.dev = DeviceVecF32.from_host(img)
        assert self.dev.ptr % 16 == 0
        self.ptr = C.c_void_p(self.dev.ptr + 4 * lead)
        self.layout = COL if col_major else ROW

    def read(self):
        """the matrix as it is now; asserts that every guard word is untouched"""
        got = self.dev.to_host()
        body = np.zeros(got.size, dtype=bool)
        if self.nl and self.w:
            body[self.lead:self.lead + self.nl * self.ld].reshape(self.nl, self.ld)[:, :self.w] = True
        assert bits(got[~body]) == bits(self.img[~body]), "a guard word was written"
        lines = got[body].reshape(self.nl, self.w)
        return lines.T if self.col_major else lines


def mulacc(a, rhs, out, accumulate):
    _ffi.check(_ffi.lib.sprs_hip_csmat_mulacc_dense_f32(a._h, rhs.ptr, rhs.shape[0], rhs.shape[1], rhs.layout, rhs.ld, out.ptr,
                                                        out.shape[0], out.layout, out.ld, 1 if accumulate else 0, None))


def check_exact(m, k, seed=1, rhs_kw=None, out_kw=None, storage=CSR, handle=None):
    """operator and accumulate form through sprs_hip_csmat_mulacc_dense_f32 against the reference chain, bit for bit; empty
    rows +0.0f / untouched (a -0.0f and a NaN planted there); guards intact.  m is the CSR form; returns the handle."""
    shape, ip, ix, dt = m
    rhs_kw, out_kw = rhs_kw or {}, out_kw or {}
    a = handle if handle is not None else DeviceCsMatF32.from_host(shape, ip, ix, dt)
    rhs = int_mat((shape[1], k), seed)
    out0 = int_mat((shape[0], k), seed + 1)
    empty = np.flatnonzero(np.diff(ip.astype(np.int64)) == 0)
    if empty.size and k:
        out0[empty[0], 0] = np.float32(-0.0)
        out0[empty[-1], k - 1] = np.float32(np.nan)
    want = spmm_f32_ref.mul_dense(shape, ip, ix, dt, rhs)
    want_acc = spmm_f32_ref.csr_mulacc_dense_rowmaj(shape, ip, ix, dt, rhs, out0.copy())
    d_rhs = Guarded(rhs, **rhs_kw)
    d_out = Guarded(np.full((shape[0], k), np.nan, dtype=np.float32), **out_kw)       # the operator form overwrites every element
    mulacc(a, d_rhs, d_out, False)
    got = d_out.read()
    assert got.dtype == np.float32 and bits(got) == bits(want)
    assert bits(got[empty]) == bits(np.zeros((empty.size, k), dtype=np.float32))        # +0.0f
    d_acc = Guarded(out0, **out_kw)
    mulacc(a, d_rhs, d_acc, True)
    got_acc = d_acc.read()
    assert bits(got_acc) == bits(want_acc)
    assert bits(got_acc[empty]) == bits(out0[empty])
    assert bits(d_rhs.read()) == bits(rhs)
    return a


SEAMS = [0, 3, 70, 1, 300, 0, 0, 9, 31, 32, 33, 1, 1, 0, 64, 127, 2]      # 674 entries: 3 tiles, rows across runs and tiles, empties


# ---- exact cases --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", K_CLASSES)
def test_exact_k_classes(k, pair, mode):
    check_exact(int_csr(SEAMS, 400, seed=k), k, seed=k)


ENTRY_COUNTS = {"1": 1, "3": 3, "T-1": T - 1, "T": T, "T+1": T + 1, "4T-1": 4 * T - 1, "4T": 4 * T, "4T+1": 4 * T + 1, "2T+3": 2 * T + 3}


@pytest.mark.parametrize("which", list(ENTRY_COUNTS))
def test_exact_entry_counts(which, pair, mode):
    nnz = ENTRY_COUNTS[which]
    check_exact(int_csr(lengths_to(nnz), 97, seed=nnz), 9, seed=nnz)
    check_exact(int_csr(lengths_to(nnz, pattern=(70, 0, 1, 300, 2)), 301, seed=nnz + 1), 16, seed=nnz)


def test_exact_row_inside_a_run_and_across_runs(pair, mode):
    # k = 16: runs of 64 (scalar) / 32 (paired) entries; k = 64: one run of 256 (scalar) / two of 128 (paired)
    lens = [5, 20, 7, 40, 3, 30, 60, 2, 100, 1, 0, 120, 9]
    for k in (16, 64):
        check_exact(int_csr(lens, 130, seed=3), k, seed=4)


@pytest.mark.parametrize("tail", [[], [0, 0, 0], [0, 5, 0]], ids=["last-row", "empty-rows-after", "rows-after"])
def test_exact_row_ends_on_a_tile_boundary(tail, pair, mode):
    check_exact(int_csr([T - 5, T + 5, 7, T - 7, T] + tail, T + 50, seed=23), 12, seed=5)
    check_exact(int_csr([T] + tail, T, seed=24), 8, seed=6)


def test_exact_fixup_spans(pair, mode):
    """a row spanning FIX_SPAN tiles beyond its first (the lane-group fix-up) and one spanning FIX_SPAN + 2 (the whole wave)"""
    lens = [3, 2300, 1, 2816, 0, 7, 300, 4096, 2]
    shape, ip, ix, dt = int_csr(lens, 4100, seed=31)
    span = lambda r: (int(ip[r + 1]) - 1) // T - int(ip[r]) // T
    assert span(1) == FIX_SPAN and span(3) == FIX_SPAN + 2 and int(ip[3]) % T == 0
    for k in (5, 16):
        check_exact((shape, ip, ix, dt), k, seed=7)


def test_exact_more_row_starts_in_a_tile_than_lanes(pair, mode):
    lens = [1, 0] * 40 + [1] * T + [0, 0, 1] * 100 + [0] * 70 + [1] * 5
    check_exact(int_csr(lens, 50, seed=41), 10, seed=8)


@pytest.mark.parametrize("cols", [4096, 4097, 8191, 12289])
def test_exact_relaid_rhs_blocks(cols, pair):
    """the re-laid-out copy in blocks of 4096 rows: a full block, one row into the second, one short of two, into the fourth"""
    lens = np.array(lengths_to(700, pattern=(3, 0, 70, 1, 200, 0, 9)))
    shape, ip, ix, dt = int_csr(lens, cols, seed=cols)
    ix = ix.copy()
    ix[-1] = cols - 1                                    # the last row's last entry: the last row of the rhs
    last = np.flatnonzero(lens)[-1]
    assert np.all(np.diff(ix[int(ip[last]):].astype(np.int64)) > 0)
    sprs_amd.set_option("spmm_relayout", 1)
    try:
        for k in (9, 32):
            check_exact((shape, ip, ix, dt), k, seed=9)
    finally:
        sprs_amd.set_option("spmm_relayout", 0)


@pytest.mark.parametrize("idx,ptr", WIDTHS)
def test_exact_index_widths(idx, ptr, pair, mode):
    check_exact(int_csr(SEAMS, 400, seed=51, idx=idx, ptr=ptr), 11, seed=10)


ELIGIBILITY = {
    "odd-ld": (dict(ld=19), {}),                          # a row-major rhs with an odd pitch: scalar lanes
    "even-ld-odd-base": (dict(ld=20, lead=9), {}),        # an even pitch, the base 4 bytes off an 8-byte boundary: scalar lanes
    "even-ld": (dict(ld=20), dict(ld=22)),                # eligible: 8-byte gathers and 8-byte result stores
    "even-ld-odd-out-base": (dict(ld=20), dict(ld=22, lead=9)),   # eligible rhs, result stored column by column
    "odd-out-ld": (dict(ld=20), dict(ld=21)),
    "colmaj-rhs": (dict(col_major=True, ld=407), {}),     # re-laid out by the auto rule: eligible through the copy
    "colmaj-out": ({}, dict(col_major=True, ld=23)),
    "colmaj-both": (dict(col_major=True), dict(col_major=True)),
}


@pytest.mark.parametrize("case", list(ELIGIBILITY))
@pytest.mark.parametrize("k", [8, 17, 18])
def test_exact_paired_form_eligibility(case, k, pair):
    rhs_kw, out_kw = ELIGIBILITY[case]
    check_exact(int_csr(SEAMS, 400, seed=61), k, seed=11, rhs_kw=rhs_kw, out_kw=out_kw)


@pytest.mark.parametrize("extra", [4096, 4097])
def test_exact_hypersparse_threshold(extra, pair):
    """rows = 4 nnz + 4096 (the tiles zero the empty rows) and + 4097 (one clear of `out`, then the accumulate form)"""
    lens = np.zeros(4 * 12 + extra, dtype=np.int64)
    lens[[5, 6, 2000, 4100]] = [3, 1, 7, 1]
    assert lens.sum() == 12
    for k, out_kw in ((3, dict(col_major=True)), (16, {}), (9, dict(ld=12)), (9, dict(col_major=True, ld=lens.size + 3))):
        check_exact(int_csr(lens, 40, seed=71), k, seed=12, out_kw=out_kw)


def test_exact_degenerate_operands(pair, mode):
    z = lambda n, dt: np.zeros(n, dtype=dt)
    check_exact(((5, 7), z(6, np.uint32), z(0, np.uint32), z(0, np.float32)), 9, seed=13)                   # nothing stored
    check_exact(((5, 7), z(6, np.uint32), z(0, np.uint32), z(0, np.float32)), 3, seed=13, out_kw=dict(col_major=True))
    check_exact(((0, 7), z(1, np.uint32), z(0, np.uint32), z(0, np.float32)), 9, seed=14)                   # no rows
    check_exact(((4, 0), z(5, np.uint32), z(0, np.uint32), z(0, np.float32)), 9, seed=15)                   # no columns
    check_exact(int_csr(SEAMS, 400, seed=16), 0, seed=16)                                                   # k = 0


@pytest.mark.parametrize("idx,ptr", [WIDTHS[0], WIDTHS[3]])
def test_csc_lhs_through_the_four_mulacc_functions(idx, ptr, pair, mode):
    shape, ip, ix, dt = int_csr(lengths_to(T + 300, pattern=(3, 0, 70, 1, 200, 0, 9)), 500, seed=81, idx=idx, ptr=ptr)
    _, cp, ci, cd = f32_ref.csc_to_csr(shape[::-1], ip, ix, dt)             # the CSC arrays of the same matrix
    a_csr = DeviceCsMatF32.from_host(shape, ip, ix, dt)
    a_csc = DeviceCsMatF32.from_host(shape, cp.astype(ptr), ci.astype(idx), cd, storage=CSC)
    for k in (3, 12):
        rhs, out0 = int_mat((shape[1], k), 82), int_mat((shape[0], k), 83)
        want = spmm_f32_ref.csr_mulacc_dense_rowmaj(shape, ip, ix, dt, rhs, out0.copy())
        for a, fns in ((a_csr, (prod.csr_mulacc_dense_rowmaj, prod.csr_mulacc_dense_colmaj)),
                       (a_csc, (prod.csc_mulacc_dense_rowmaj, prod.csc_mulacc_dense_colmaj))):
            for fn, col_major in zip(fns, (False, True)):
                res = prod.DeviceMatF32.from_host(out0, col_major=col_major)
                fn(a, prod.DeviceMatF32.from_host(rhs, col_major=col_major), res)
                got = res.to_host()
                assert got.dtype == np.float32 and bits(np.ascontiguousarray(got)) == bits(want)
        check_exact((shape, ip, ix, dt), k, seed=84, handle=a_csc)           # guards, both forms, the cached CSR form


def test_colmaj_arm_below_8_columns_is_the_spmv_column_by_column(pair):
    """column-major x column-major with k < 8 runs through spmv_f32: on ROUNDED data the bits of `&A * &x` per column"""
    rng = np.random.default_rng(91)
    shape, ip, ix, _ = int_csr(lengths_to(3 * T + 40, pattern=(3, 0, 70, 1, 200, 0, 9)), 500, seed=92)
    dt = (rng.random(ix.size) + 0.5).astype(np.float32)
    _, cp, ci, cd = f32_ref.csc_to_csr(shape[::-1], ip, ix, dt)
    for a in (DeviceCsMatF32.from_host(shape, ip, ix, dt), DeviceCsMatF32.from_host(shape, cp.astype(np.uint32), ci.astype(np.uint32), cd, storage=CSC)):
        for k in (1, 7):
            rhs = (rng.random((shape[1], k)) - 0.5).astype(np.float32)
            out = prod.csmat_mul_dense(a, prod.DeviceMatF32.from_host(rhs, col_major=True))
            assert out.col_major
            cols = [(a * DeviceVecF32.from_host(np.ascontiguousarray(rhs[:, j]))).to_host() for j in range(k)]
            assert bits(np.ascontiguousarray(out.to_host())) == bits(np.stack(cols, axis=1))
            out0 = (rng.random((shape[0], k)) - 0.5).astype(np.float32)
            res = prod.DeviceMatF32.from_host(out0, col_major=True)
            (prod.csc_mulacc_dense_colmaj if a.is_csc() else prod.csr_mulacc_dense_colmaj)(a, prod.DeviceMatF32.from_host(rhs, col_major=True), res)
            acc = []
            for j in range(k):
                y = DeviceVecF32.from_host(np.ascontiguousarray(out0[:, j]))
                (prod.mul_acc_mat_vec_csc if a.is_csc() else prod.mul_acc_mat_vec_csr)(a, DeviceVecF32.from_host(np.ascontiguousarray(rhs[:, j])), y)
                acc.append(y.to_host())
            assert bits(np.ascontiguousarray(res.to_host())) == bits(np.stack(acc, axis=1))


@pytest.mark.parametrize("storage", [CSR, CSC])
def test_csmat_mul_dense_result_layout(storage, pair):
    shape, ip, ix, dt = int_csr(SEAMS, 400, seed=101)
    if storage == CSC:
        _, cp, ci, cd = f32_ref.csc_to_csr(shape[::-1], ip, ix, dt)
        a = DeviceCsMatF32.from_host(shape, cp.astype(np.uint32), ci.astype(np.uint32), cd, storage=CSC)
    else:
        a = DeviceCsMatF32.from_host(shape, ip, ix, dt)
    for k in (7, 8):
        rhs = int_mat((shape[1], k), 102)
        want = spmm_f32_ref.mul_dense(shape, ip, ix, dt, rhs)
        for col_major in (False, True):
            for out in (a * prod.DeviceMatF32.from_host(rhs, col_major=col_major), a @ prod.DeviceMatF32.from_host(rhs, col_major=col_major)):
                assert isinstance(out, prod.DeviceMatF32) and isinstance(out.vec, DeviceVecF32)
                assert out.col_major == spmm_f32_ref.result_col_major(k) == (k < 8)
                assert bits(np.ascontiguousarray(out.to_host())) == bits(want)


@pytest.mark.parametrize("storage", [CSR, CSC])
def test_dense_dot_csmat_against_numpy(storage, pair):
    shape, ip, ix, dt = int_csr(SEAMS, 400, seed=111)
    dense = np.zeros(shape, dtype=np.float64)
    dense[np.repeat(np.arange(shape[0]), np.diff(ip.astype(np.int64))), ix.astype(np.int64)] = dt
    if storage == CSC:
        _, cp, ci, cd = f32_ref.csc_to_csr(shape[::-1], ip, ix, dt)
        a = DeviceCsMatF32.from_host(shape, cp.astype(np.uint32), ci.astype(np.uint32), cd, storage=CSC)
    else:
        a = DeviceCsMatF32.from_host(shape, ip, ix, dt)
    for nrows in (5, 9):                                  # the transposed product has nrows columns: both result layouts
        lhs = int_mat((nrows, shape[0]), 112)
        want = (lhs.astype(np.float64) @ dense).astype(np.float32)          # exact: integers below 2^24
        for col_major in (False, True):
            out = prod.dense_dot_csmat(prod.DeviceMatF32.from_host(lhs, col_major=col_major), a)
            assert isinstance(out, prod.DeviceMatF32) and out.col_major == (nrows >= 8)       # reversed_axes of the transposed product
            assert bits(np.ascontiguousarray(out.to_host())) == bits(want)
        again = prod.dense_dot_csmat(prod.DeviceMatF32.from_host(lhs), a)                     # the view kept in the handle
        assert bits(np.ascontiguousarray(again.to_host())) == bits(want)
    a.refresh()
    assert bits(np.ascontiguousarray(prod.dense_dot_csmat(prod.DeviceMatF32.from_host(lhs), a).to_host())) == bits(want)


# ---- rounded arithmetic ----------------------------------------------------------------------------------------------------
def _signed(data, seed):
    rng = np.random.default_rng(seed)
    return ((rng.random(len(data)) + 0.5) * rng.choice([-1.0, 1.0], size=len(data))).astype(np.float32)


def _row_sums(ip64, v):
    """per-row sums of the n x k array v (float64) over the rows' entries"""
    m = np.diff(ip64)
    s = np.add.reduceat(np.concatenate([v, np.zeros((1, v.shape[1]))]), ip64[:-1], axis=0)
    return np.where((m > 0)[:, None], s, 0.0)


def _check_bound(shape, ip, ix, dt, k, seed):
    """every element: |out - s| <= gamma_m S + slack (operator form), |out - (s + out0)| <= gamma_{m+1} (S + |out0|) + slack
    (accumulate form), slack = m 2^-52 S (the float64 reference sum's own error); under spmm_long_row = 2048 the rows of <= 2048
    entries equal the numpy chain bit for bit in both forms.  Prints the worst ratio before it asserts."""
    rng = np.random.default_rng(seed)
    ip64, ix64 = ip.astype(np.int64), ix.astype(np.int64)
    m = np.diff(ip64).astype(np.float64)[:, None]
    rhs = ((rng.random((shape[1], k)) + 0.5) * rng.choice([-1.0, 1.0], size=(shape[1], k))).astype(np.float32)
    out0 = ((rng.random((shape[0], k)) + 0.5) * rng.choice([-1.0, 1.0], size=(shape[0], k))).astype(np.float32)
    p = dt.astype(np.float64)[:, None] * rhs.astype(np.float64)[ix64]
    S, s = _row_sums(ip64, np.abs(p)), _row_sums(ip64, p)
    slack = m * 2.0 ** -52 * S
    gamma = m * U / (1.0 - m * U)
    gamma1 = (m + 1) * U / (1.0 - (m + 1) * U)
    empty = m[:, 0] == 0
    o64 = out0.astype(np.float64)
    a = DeviceCsMatF32.from_host(shape, ip, ix, dt)
    d_rhs = prod.DeviceMatF32.from_host(rhs)

    def run():
        y = (a * d_rhs).to_host()
        res = prod.DeviceMatF32.from_host(out0)
        prod.csr_mulacc_dense_rowmaj(a, d_rhs, res)
        return y, res.to_host()
    for pair_form in (2, 1, 0):
        sprs_amd.set_option("spmm_f32_pair", pair_form)
        try:
            y, ya = run()
        finally:
            sprs_amd.set_option("spmm_f32_pair", 1)
        err, erra = np.abs(y.astype(np.float64) - s), np.abs(ya.astype(np.float64) - (s + o64))
        worst = np.max((err - slack) / np.maximum(gamma * S, 1e-300), initial=0.0, where=m > 0)
        worsta = np.max((erra - slack) / np.maximum(gamma1 * (S + np.abs(o64)), 1e-300), initial=0.0, where=m > 0)
        print("k = %d, pair = %d: worst |out - s| / (gamma_m S) = %.3g, accumulate form %.3g, over %d rows" % (k, pair_form, worst, worsta, shape[0]))
        assert np.all(err <= gamma * S + slack)
        assert np.all(erra <= gamma1 * (S + np.abs(o64)) + slack)
        assert bits(y[empty]) == bits(np.zeros((int(empty.sum()), k), dtype=np.float32))
        assert bits(ya[empty]) == bits(out0[empty])
    sprs_amd.set_option("spmm_long_row", 2048)
    try:
        y, ya = run()
    finally:
        sprs_amd.set_option("spmm_long_row", -1)
    short = m[:, 0] <= 2048
    want = spmm_f32_ref.mul_dense(shape, ip, ix, dt, rhs, max_len=2048)
    want_acc = spmm_f32_ref.csr_mulacc_dense_rowmaj(shape, ip, ix, dt, rhs, out0.copy(), max_len=2048)
    assert bits(y[short]) == bits(want[short]) and bits(ya[short]) == bits(want_acc[short])
    assert np.all(np.abs(y.astype(np.float64) - s) <= gamma * S + slack)                  # the long rows: the chunk kernels
    assert np.all(np.abs(ya.astype(np.float64) - (s + o64)) <= gamma1 * (S + np.abs(o64)) + slack)


@pytest.mark.parametrize("k", [16, 33])
def test_rounded_rmat(k):
    n = 3000 if EMULATED else 60000
    ip, ix, dt = gen.rmat_csr(n, 16)
    ip, ix = ip.numpy().astype(np.uint64), ix.numpy().astype(np.uint32)
    _check_bound((n, n), ip, ix, _signed(dt.numpy(), 51), k, 52)


def test_rounded_ragged():
    rng = np.random.default_rng(53)
    nrows = 4 if EMULATED else 36
    lengths = np.concatenate([rng.integers(0, 5001, size=nrows), [0, 5000, 1, 0, 2048, 2049]])
    shape, ip, ix, dt = ragged_csr(lengths, 20000, seed=54, idx=np.uint32, ptr=np.uint64)
    assert EMULATED or 80_000 < ix.size < 130_000
    _check_bound(shape, ip, ix, _signed(dt, 55), 8, 56)


# ---- the reference's golden products -----------------------------------------------------------------------------------------
def test_golden_products(golden):
    """prod.rs:502-542 cast to f32: mat1 x mat_dense1 (epsilon 0 there) survives the cast exactly and must match bit for bit;
    mat5 x mat_dense2 by the gamma bound"""
    from conftest import as_csr
    shape, ip, ix, dt = as_csr(golden["mat1"], np.uint32, np.uint32)
    dense, exp = np.array(golden["mat_dense1"]), np.array(golden["mat1_times_mat_dense1"]["rows"])
    assert golden["mat1_times_mat_dense1"]["epsilon"] == 0
    d32, r32, e32 = dt.astype(np.float32), dense.astype(np.float32), exp.astype(np.float32)
    assert np.array_equal(d32.astype(np.float64), dt) and np.array_equal(r32.astype(np.float64), dense) and np.array_equal(e32.astype(np.float64), exp)
    a = DeviceCsMatF32.from_host(shape, ip, ix, d32)
    b = prod.DeviceMatF32.from_host(r32)
    res = prod.DeviceMatF32(exp.shape[0], exp.shape[1])
    prod.csr_mulacc_dense_rowmaj(a, b, res)
    assert bits(res.to_host()) == bits(e32)
    out = a * b
    assert out.col_major and bits(np.ascontiguousarray(out.to_host())) == bits(e32)      # 5 columns: `.f()` layout
    shape, ip, ix, dt = as_csr(golden["mat5"], np.uint32, np.uint32)
    d32, r32 = dt.astype(np.float32), np.array(golden["mat_dense2"]).astype(np.float32)
    got = (DeviceCsMatF32.from_host(shape, ip, ix, d32) * prod.DeviceMatF32.from_host(r32)).to_host().astype(np.float64)
    ip64 = ip.astype(np.int64)
    p = d32.astype(np.float64)[:, None] * r32.astype(np.float64)[ix.astype(np.int64)]
    m = np.diff(ip64).astype(np.float64)[:, None]
    S, s = _row_sums(ip64, np.abs(p)), _row_sums(ip64, p)
    assert np.all(np.abs(got - s) <= m * U / (1.0 - m * U) * S + m * 2.0 ** -52 * S)


# ---- determinism, streams -----------------------------------------------------------------------------------------------------
def test_five_runs_on_one_handle_give_the_same_bits(pair, mode):
    rng = np.random.default_rng(121)
    lens = np.concatenate([rng.integers(0, 60, size=300), [2300, 0, 700]])
    shape, ip, ix, dt = ragged_csr(lens, 3000, seed=122, idx=np.uint32, ptr=np.uint32)
    a = DeviceCsMatF32.from_host(shape, ip, ix, _signed(dt, 123))
    rhs = prod.DeviceMatF32.from_host((rng.random((shape[1], 20)) - 0.5).astype(np.float32))
    first = bits((a * rhs).to_host())
    for _ in range(4):
        assert bits((a * rhs).to_host()) == first


@pytest.mark.parametrize("stream_mode", [1, 0])
def test_plan_built_on_a_nonblocking_stream(stream_mode):
    """the SpMM plan made by a product on a torch stream (hipStreamNonBlocking) and used there at once is the plan of the null
    stream: same bits as a handle planned on the null stream, in both decompositions"""
    import torch
    n, k = 30000, 8
    indptr, indices, data = gen.rmat_csr(n, 10, seed=13)
    ip, ix, dt = indptr.numpy().astype(np.uint64), indices.numpy().astype(np.uint32), _signed(data.numpy(), 131)
    rhs = prod.DeviceMatF32.from_host((np.random.default_rng(5).random((n, k)) + 0.5).astype(np.float32))
    s = torch.cuda.Stream(device=torch.device("cuda", 0))
    out = []
    sprs_amd.set_option("spmm_stream", stream_mode)
    try:
        for stream in (s, None):
            a = DeviceCsMatF32.from_host((n, n), ip, ix, dt)
            res = prod.DeviceMatF32.from_host(np.zeros((n, k), dtype=np.float32))
            prod.csr_mulacc_dense_rowmaj(a, rhs, res, stream=stream)    # the plan is built and used on `stream`
            if stream is not None:
                stream.synchronize()
            out.append(res.to_host())
    finally:
        sprs_amd.set_option("spmm_stream", 1)
    assert np.any(out[0] != 0) and bits(out[0]) == bits(out[1])


# ---- contracts ------------------------------------------------------------------------------------------------------------------
def test_contract_violations():
    shape, ip, ix, dt = int_csr([3, 0, 5, 1, 0, 2, 7], 9, seed=3)          # 7 x 9
    a = DeviceCsMatF32.from_host(shape, ip, ix, dt)
    c = a.to_other_storage()
    M = prod.DeviceMatF32
    with pytest.raises(_ffi.SprsHipError, match="Dimension mismatch") as e:         # prod.rs:199-201
        prod.csr_mulacc_dense_rowmaj(a, M(8, 3), M(7, 3))
    assert e.value.status == _ffi.DIM_MISMATCH
    with pytest.raises(_ffi.SprsHipError, match="Dimension mismatch"):
        prod.csr_mulacc_dense_rowmaj(a, M(9, 3), M(7, 2))
    with pytest.raises(_ffi.SprsHipError, match="Storage mismatch") as e:           # prod.rs:202
        prod.csr_mulacc_dense_rowmaj(c, M(9, 2), M(7, 2))
    assert e.value.status == _ffi.STORAGE_MISMATCH
    with pytest.raises(_ffi.SprsHipError, match="Dimension mismatch"):              # both wrong: the dimensions are reported
        prod.csr_mulacc_dense_rowmaj(c, M(8, 2), M(7, 2))
    with pytest.raises(_ffi.SprsHipError, match="Dimension mismatch"):
        prod.csc_mulacc_dense_colmaj(a, M(8, 2), M(7, 2))
    call = _ffi.lib.sprs_hip_csmat_mulacc_dense_f32
    rhs, out = DeviceVecF32.zeros(9 * 4), DeviceVecF32.zeros(7 * 4)
    rp, op = C.c_void_p(rhs.ptr), C.c_void_p(out.ptr)

    def status(*args):
        st = call(*args)
        return st, _ffi.lib.sprs_hip_last_error().decode()
    # the library itself: dimensions before storage (the CSC handle through the CSR-only entry)
    st, msg = status(a._h, rp, 8, 4, ROW, 4, op, 7, ROW, 4, 1, None)
    assert st == _ffi.DIM_MISMATCH and "Dimension mismatch" in msg
    st, msg = _ffi.lib.sprs_hip_spmm_rowmaj_f32(c._h, rp, 8, 4, 4, op, 7, 4, 1, None), _ffi.lib.sprs_hip_last_error().decode()
    assert st == _ffi.DIM_MISMATCH and "Dimension mismatch" in msg
    st, msg = _ffi.lib.sprs_hip_spmm_rowmaj_f32(c._h, rp, 9, 4, 4, op, 7, 4, 1, None), _ffi.lib.sprs_hip_last_error().decode()
    assert st == _ffi.STORAGE_MISMATCH and "Storage mismatch" in msg
    st, msg = status(a._h, rp, 9, 4, 2, 4, op, 7, ROW, 4, 1, None)
    assert st == _ffi.INVALID_ARG and "bad layout tag" in msg
    st, msg = status(a._h, rp, 9, 4, ROW, 4, op, 7, -1, 4, 1, None)
    assert st == _ffi.INVALID_ARG and "bad layout tag" in msg
    for args in ((a._h, rp, 9, 4, ROW, 3, op, 7, ROW, 4, 1, None), (a._h, rp, 9, 4, ROW, 4, op, 7, ROW, 3, 1, None),
                 (a._h, rp, 9, 4, COL, 8, op, 7, ROW, 4, 1, None), (a._h, rp, 9, 4, ROW, 4, op, 7, COL, 6, 1, None)):
        st, msg = status(*args)
        assert st == _ffi.INVALID_ARG and "leading dimension smaller" in msg
    st, msg = status(a._h, None, 9, 4, ROW, 4, op, 7, ROW, 4, 1, None)
    assert st == _ffi.INVALID_ARG and "NULL matrix" in msg
    st, msg = status(a._h, rp, 9, 4, ROW, 4, None, 7, ROW, 4, 1, None)
    assert st == _ffi.INVALID_ARG and "NULL matrix" in msg
    st, msg = status(None, rp, 9, 4, ROW, 4, op, 7, ROW, 4, 1, None)
    assert st == _ffi.INVALID_ARG and "NULL handle" in msg
    lay = C.c_int32(0)
    assert _ffi.lib.sprs_hip_csmat_mul_dense_f32(a._h, rp, 9, 4, ROW, 4, op, None, None) == _ffi.INVALID_ARG
    assert _ffi.lib.sprs_hip_dense_dot_csmat_f32(rp, 4, 7, 3, 7, a._h, op, C.byref(lay), None) == _ffi.INVALID_ARG
    assert _ffi.lib.sprs_hip_dense_dot_csmat_f32(rp, 4, 7, ROW, 7, None, op, C.byref(lay), None) == _ffi.INVALID_ARG


def test_out_overlapping_rhs_and_the_disjoint_views():
    sq = DeviceCsMatF32.from_host((6, 6), np.arange(7, dtype=np.uint32), np.arange(6, dtype=np.uint32), np.ones(6, dtype=np.float32))
    buf = prod.DeviceMatF32(6, 4)
    with pytest.raises(_ffi.SprsHipError) as e:
        prod.csr_mulacc_dense_rowmaj(sq, buf, buf)
    assert e.value.status == _ffi.INVALID_ARG and "overlaps" in str(e.value)
    # two element-disjoint views of ONE buffer: rhs = buf[:, 0:k], out = buf[:, k:2k] with pitch 2k (row-major), and the same
    # as column blocks (column-major)
    rng = np.random.default_rng(141)
    scale = np.array([1, 2, 3, 4, 5, 6], dtype=np.float32)
    sq2 = DeviceCsMatF32.from_host((6, 6), np.arange(7, dtype=np.uint32), np.array([5, 4, 3, 2, 1, 0], dtype=np.uint32), scale)   # a scaled row reversal
    call = _ffi.lib.sprs_hip_csmat_mulacc_dense_f32
    for layout, ld in ((ROW, 8), (COL, 12)):
        host = rng.integers(-8, 9, size=48).astype(np.float32)
        both = DeviceVecF32.from_host(host)
        off = 4 if layout == ROW else 6
        _ffi.check(call(sq2._h, C.c_void_p(both.ptr), 6, 4, layout, ld, C.c_void_p(both.ptr + off * 4), 6, layout, ld, 0, None))
        got = both.to_host()
        if layout == ROW:
            v = got.reshape(6, 8)
            src, dst = host.reshape(6, 8)[:, :4], v[:, 4:]
            assert bits(v[:, :4]) == bits(src)
        else:
            v = got.reshape(4, 12).T
            src, dst = host.reshape(4, 12).T[:6, :], v[6:, :]
            assert bits(v[:6, :]) == bits(src)
        assert bits(dst) == bits(scale[:, None] * src[::-1, :])
        st = call(sq2._h, C.c_void_p(both.ptr), 6, 4, layout, ld, C.c_void_p(both.ptr + (off - 1) * 4), 6, layout, ld, 0, None)
        assert st == _ffi.INVALID_ARG                      # the same pitch with views that DO share elements


def test_mixed_precision_is_a_type_error_in_every_python_entry():
    shape, ip, ix, dt = int_csr([3, 0, 5, 1, 0, 2, 7], 9, seed=3)
    a32 = DeviceCsMatF32.from_host(shape, ip, ix, dt)
    a64 = a32.to_f64()
    c32, c64 = a32.to_other_storage(), a64.to_other_storage()
    r32, r64 = prod.DeviceMatF32(9, 8), prod.DeviceMat(9, 8)
    o32, o64 = prod.DeviceMatF32(7, 8), prod.DeviceMat(7, 8)
    l32, l64 = prod.DeviceMatF32(4, 7), prod.DeviceMat(4, 7)
    for fn, m32, m64 in ((prod.csr_mulacc_dense_rowmaj, a32, a64), (prod.csr_mulacc_dense_colmaj, a32, a64),
                         (prod.csc_mulacc_dense_rowmaj, c32, c64), (prod.csc_mulacc_dense_colmaj, c32, c64)):
        for args in ((m32, r64, o32), (m32, r32, o64), (m32, r64, o64), (m64, r32, o64), (m64, r64, o32), (m64, r32, o32)):
            with pytest.raises(TypeError):
                fn(*args)
        fn(m32, r32, o32)
        fn(m64, r64, o64)
    for mat, rhs in ((a32, r64), (a64, r32)):
        with pytest.raises(TypeError):
            prod.csmat_mul_dense(mat, rhs)
        with pytest.raises(TypeError):
            mat * rhs
        with pytest.raises(TypeError):
            mat @ rhs
    for lhs, mat in ((l64, a32), (l32, a64)):
        with pytest.raises(TypeError):
            prod.dense_dot_csmat(lhs, mat)
    with pytest.raises(TypeError):
        prod.DeviceMatF32(2, 2, DeviceVec.zeros(4))        # a DeviceMatF32 never holds doubles
    with pytest.raises(TypeError):
        prod.DeviceMat(2, 2, DeviceVecF32.zeros(4))
    assert not isinstance(r32, prod.DeviceMat) and not isinstance(r64, prod.DeviceMatF32)
