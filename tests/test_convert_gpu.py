"""GPU parity tests: to_other_storage (csmat.rs:1405-1426, 1782-1829), slice_outer
(slicing.rs:65-89), transpose_view (csmat.rs:982-991) and the storage dispatch of
csmat_mul_csmat (csmat.rs:1895-1949) against the oracle / golden fixtures."""
import os

import numpy as np
import pytest

from conftest import IDX_COMBOS, as_csr
from helpers import fresh_blocks, ragged_csr

pytestmark = pytest.mark.gpu
EMULATED = bool(os.environ.get("SPRS_HIP_LIBRARY"))   # the kernel emulator of tests/emu (tests/test_convert_emu_cpu.py)


@pytest.fixture(scope="module")
def hip():
    import sprs_amd
    if sprs_amd.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X (no CPU fallback exists)")
    return sprs_amd


def dev(fx_or_tuple, storage=None, idx=np.uint64, ptr=np.uint64):
    from sprs_amd import _ffi
    from sprs_amd.device import DeviceCsMat
    if isinstance(fx_or_tuple, dict):
        shape, ip, ix, dt = as_csr(fx_or_tuple, idx, ptr)
        storage = _ffi.CSC if fx_or_tuple["storage"] == "CSC" else _ffi.CSR
    else:
        shape, ip, ix, dt = fx_or_tuple
        storage = _ffi.CSR if storage is None else storage
    return DeviceCsMat.from_host(shape, ip, ix, dt, storage=storage)


def same(d, fx, idx=np.uint64, ptr=np.uint64):
    from sprs_amd import _ffi
    shape, ip, ix, dt = d.to_host()
    e = as_csr(fx, idx, ptr)
    st = _ffi.CSC if fx["storage"] == "CSC" else _ffi.CSR
    return (d.storage() == st and tuple(shape) == tuple(e[0]) and np.array_equal(ip, e[1])
            and np.array_equal(ix, e[2]) and np.array_equal(dt, e[3]))


@pytest.mark.parametrize("idx,ptr", IDX_COMBOS)
def test_to_other_storage_golden(hip, golden, idx, ptr):
    # mat1 (CSR) <-> mat1_csc are the same matrix (test_data.rs:6-18)
    assert same(dev(golden["mat1"], idx=idx, ptr=ptr).to_other_storage(), golden["mat1_csc"], idx, ptr)
    assert same(dev(golden["mat1_csc"], idx=idx, ptr=ptr).to_other_storage(), golden["mat1"], idx, ptr)
    # rectangular: 5 x 15
    from oracle import oracle
    shape, ip, ix, dt = as_csr(golden["mat5"], idx, ptr)
    o = dev(golden["mat5"], idx=idx, ptr=ptr).to_other_storage()
    rip, rix, rdt = oracle.convert_storage(5, 15, ip, ix, dt)
    s2, gip, gix, gdt = o.to_host()
    assert o.is_csc() and tuple(s2) == (5, 15)
    assert np.array_equal(gip, rip) and np.array_equal(gix, rix) and np.array_equal(gdt, rdt)


def test_to_other_storage_rmat_and_long_columns(hip):
    from oracle import oracle
    from sprs_amd import gen
    n = 10000 if EMULATED else 40000
    indptr, indices, data = gen.rmat_csr(n, 12, seed=9)      # hub columns exceed the 1024-entry wave path
    ip, ix, dt = indptr.numpy().astype(np.uint64), indices.numpy().astype(np.uint64), data.numpy()
    o = dev(((n, n), ip, ix, dt)).to_other_storage()
    rip, rix, rdt = oracle.convert_storage(n, n, ip, ix, dt)
    _, gip, gix, gdt = o.to_host()
    assert int(np.diff(rip.astype(np.int64)).max()) > 1024
    assert np.array_equal(gip, rip) and np.array_equal(gix, rix) and np.array_equal(gdt, rdt)
    back = o.to_other_storage()                               # round trip
    _, bip, bix, bdt = back.to_host()
    assert back.is_csr() and np.array_equal(bip, ip) and np.array_equal(bix, ix) and np.array_equal(bdt, dt)
    # one column longer than one 2^19 bitmap window of the outer range
    rows = (1 << 19) + 777
    lens = np.ones(rows, dtype=np.int64)
    shape, ip, ix, dt = (rows, 3), np.arange(rows + 1, dtype=np.uint64), np.full(rows, 1, dtype=np.uint64), \
        np.arange(rows, dtype=np.float64)
    o = dev((shape, ip, ix, dt)).to_other_storage()
    _, gip, gix, gdt = o.to_host()
    assert list(gip) == [0, 0, rows, rows] and np.array_equal(gix, np.arange(rows, dtype=np.uint64))
    assert np.array_equal(gdt, dt)


def test_storage_dispatch_golden(hip, golden):
    # prod.rs:425-458: mul_csr_csr, mul_csc_csc, mul_csc_csr through `&A * &B`
    assert same(dev(golden["mat1_csc"]) * dev(golden["mat4"]), golden["mat1_csc_matprod_mat4"])   # (CSC,CSC)
    assert same(dev(golden["mat1"]) * dev(golden["mat1_csc"]), golden["mat1_self_matprod"])        # (CSR,CSC)
    r = dev(golden["mat1_csc"]) * dev(golden["mat1"])                                              # (CSC,CSR) -> CSC
    assert r.is_csc()
    assert same(r.to_other_storage(), golden["mat1_self_matprod"])


def test_gh374_index_overflow(hip):
    # tests/gh374.rs:10-33 with u32 in place of u16 cannot be allocated (2^32 rows of indptr is fine
    # on 288 GB, but not in a unit test): pin the documented status on the check itself instead —
    # a CSC-tagged handle whose `rows` exceeds u32 while the arrays stay tiny.
    import ctypes as C
    from sprs_amd import SprsHipError, _ffi
    from sprs_amd.device import DeviceCsMat
    rows = (1 << 32) + 5
    m = DeviceCsMat.from_host((rows, 1), np.array([0, 1], dtype=np.uint32), np.array([7], dtype=np.uint32),
                              np.ones(1), storage=_ffi.CSC, validate=False)
    with pytest.raises(SprsHipError, match="Index type is not large enough to hold") as e:
        m.to_other_storage()
    assert e.value.status == _ffi.INDEX_OVERFLOW


def test_slice_outer_and_transpose_view(hip, golden):
    from oracle import oracle
    a = dev(golden["mat1"])
    s = a.slice_outer(1, 4)
    shape, ip, ix, dt = s.to_host()
    e = as_csr(golden["mat1"])
    lo, hi = int(e[1][1]), int(e[1][4])
    assert tuple(shape) == (3, 5) and list(ip) == [int(v) - lo for v in e[1][1:5]]
    assert np.array_equal(ix, e[2][lo:hi]) and np.array_equal(dt, e[3][lo:hi])
    assert a.slice_outer(2, 2).nnz() == 0
    with pytest.raises(hip.SprsHipError):
        a.slice_outer(3, 9)
    t = a.transpose_view()
    assert t.is_csc() and t.shape() == (5, 5)
    # link by link: A^T as CSC shares A's arrays; converted, A^T as CSR holds the arrays of A as CSC; its transpose view
    # IS A as CSC; one more conversion is A as CSR again
    assert all(np.array_equal(x, y) for x, y in zip(t.to_host()[1:], e[1:]))
    tc = t.to_other_storage()
    c = as_csr(golden["mat1_csc"])
    assert tc.is_csr() and tc.shape() == (5, 5) and all(np.array_equal(x, y) for x, y in zip(tc.to_host()[1:], c[1:]))
    a_csc = tc.transpose_view()
    assert same(a_csc, golden["mat1_csc"])
    assert same(a_csc.to_other_storage(), golden["mat1"])
    # SpMV on a materialised slice == rows of the full product
    from sprs_amd.device import DeviceVec
    x = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
    full = (a * DeviceVec.from_host(x)).to_host()
    part = (s * DeviceVec.from_host(x)).to_host()
    assert np.array_equal(part, full[1:4])


def test_mul_csc_vec_golden(hip, golden):
    # prod.rs:325-373 mul_csc_vec / mul_csc_vec_ndarray, and `&A_csc * &x` (csmat.rs:2149-2156)
    from sprs_amd import _ffi, prod
    from sprs_amd.device import DeviceCsMat, DeviceVec
    fx = golden["mul_csc_vec"]
    shape, ip, ix, dt = as_csr(fx)
    m = DeviceCsMat.from_host(shape, ip, ix, dt, storage=_ffi.CSC)
    x = DeviceVec.from_host(np.array(fx["x"]))
    y = DeviceVec.zeros(5)
    prod.mul_acc_mat_vec_csc(m, x, y)
    assert np.all(np.abs(y.to_host() - np.array(fx["expected"])) < fx["epsilon"])
    prod.mul_acc_mat_vec_csc(m, x, y)                                   # accumulates
    assert np.all(np.abs(y.to_host() - 2 * np.array(fx["expected"])) < 2 * fx["epsilon"])
    assert np.all(np.abs((m * x).to_host() - np.array(fx["expected"])) < fx["epsilon"])
    csr = DeviceCsMat.from_host(shape, ip, ix, dt)
    with pytest.raises(hip.SprsHipError, match="Storage mismatch"):
        prod.mul_acc_mat_vec_csc(csr, x, y)


def test_gh374_literal_u16(hip):
    """sprs/tests/gh374.rs:10-33 with its own types (CsMatI<_, u16, usize>): X is 2^18 x 16 with one entry at
    (2^17, 4); `&X.transpose_view() * &X` is the (CSC, CSR) case of csmat_mul_csmat, which converts the rhs to CSC —
    row indices up to 2^17 do not fit u16: "Index type is not large enough to hold" (csmat.rs:1794-1797)."""
    from sprs_amd.device import DeviceCsMat
    rows, cols = 1 << 18, 1 << 4
    ip = np.zeros(rows + 1, dtype=np.uint64)
    ip[(1 << 17) + 1:] = 1
    x = DeviceCsMat.from_host((rows, cols), ip, np.array([1 << 2], dtype=np.uint16), np.array([1.0]))
    assert x.index_bytes() == 2 and x.indptr_bytes() == 8 and x.nnz() == 1
    shape, gip, gix, gdt = x.to_host()
    assert gix.dtype == np.uint16 and gix.tolist() == [4] and np.array_equal(gip, ip)
    with pytest.raises(hip.SprsHipError) as e:
        x.transpose_view() * x
    assert e.value.status == hip._ffi.INDEX_OVERFLOW
    assert "Index type is not large enough to hold" in str(e.value)
    # the other way round everything fits: X * X^T is (CSR, CSC) -> 2^18 x 2^18 with one entry, u16 columns cannot hold 2^17
    with pytest.raises(hip.SprsHipError) as e:
        x * x.transpose_view()
    assert e.value.status == hip._ffi.INDEX_OVERFLOW


@pytest.mark.parametrize("idx,ptr", [(np.uint16, np.uint16), (np.uint16, np.uint64), (np.uint32, np.uint16)])
def test_two_byte_index_types(hip, golden, idx, ptr):
    """SpIndex covers u16 / i16 (indexing.rs:124-130): 2-byte host arrays are widened on upload and narrowed on
    download; SpMV, the product and its storage dispatch, the conversion and slices give the golden results with
    the declared index types; results that do not fit them are refused."""
    from sprs_amd.device import DeviceCsMat, DeviceVec
    a = as_csr(golden["mat1"], idx, ptr)
    b = as_csr(golden["mat2"], idx, ptr)
    A, B = DeviceCsMat.from_host(*a), DeviceCsMat.from_host(*b)
    assert A.index_bytes() == np.dtype(idx).itemsize and A.indptr_bytes() == np.dtype(ptr).itemsize
    for x, y in zip(A.to_host()[1:], a[1:]):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    exp = as_csr(golden["mat1_matprod_mat2"], idx, ptr)
    got = (A * B).to_host()
    for x, y in zip(got[1:], exp[1:]):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    # storage dispatch with a CSC rhs: same matrix, same result (prod.rs:438-458)
    got2 = (A * B.to_other_storage()).to_host()
    for x, y in zip(got2[1:], exp[1:]):
        assert np.array_equal(x, y)
    fx = golden["mul_csr_vec"]
    shape, ip, ix, dt = as_csr(fx, idx, ptr)
    y = (DeviceCsMat.from_host(shape, ip, ix, dt) * DeviceVec.from_host(np.array(fx["x"]))).to_host()
    assert np.all(np.abs(y - np.array(fx["expected"])) < fx["epsilon"])
    sl = A.slice_outer(1, 4)
    sip, six, sdt = A.slice_outer_to_host(1, 4)
    assert six.dtype == np.dtype(idx) and np.array_equal(sl.to_host()[2], six)
    if np.dtype(ptr).itemsize == 2:
        # nnz of a product above 65535 does not fit a u16 indptr (Iptr::from_usize, smmp.rs:121)
        n, w = 1000, 40                                           # band of 41: 40 k entries fit, the product's 80 k do not
        lens = np.minimum(w + 1, n - np.arange(n))
        bip = np.zeros(n + 1, dtype=np.int64)
        bip[1:] = np.cumsum(lens)
        bix = np.concatenate([np.arange(i, i + l) for i, l in enumerate(lens)])
        assert bip[-1] <= 0xFFFF
        band = DeviceCsMat.from_host((n, n), bip.astype(np.uint16), bix.astype(idx), np.ones(bix.size))
        with pytest.raises(hip.SprsHipError) as e:
            band * band
        assert e.value.status == hip._ffi.INDEX_OVERFLOW


# ---- seams of the conversion, the scan behind it and slice_outer: bit-exact against the oracle ---------------------

def csr_from_cells(outer, inner, o, c, seed, idx=np.uint64, ptr=np.uint64):
    """CSR arrays of the distinct cells (o, c), normal values"""
    o, c = np.asarray(o, dtype=np.int64), np.asarray(c, dtype=np.int64)
    order = np.lexsort((c, o))
    o, c = o[order], c[order]
    assert not np.any((o[1:] == o[:-1]) & (c[1:] == c[:-1]))
    ip = np.zeros(outer + 1, dtype=np.int64)
    np.cumsum(np.bincount(o, minlength=outer), out=ip[1:])
    return (outer, inner), ip.astype(ptr), c.astype(idx), np.random.default_rng(seed).standard_normal(c.size)


def check_conversion(m, idx, ptr, storage=None):
    """to_other_storage of the (outer x inner) arrays m == the oracle's, dtypes included, and the way back gives m's bits.
    Returns the converted arrays."""
    from oracle import oracle
    from sprs_amd import _ffi
    storage = _ffi.CSR if storage is None else storage
    (outer, inner), ip, ix, dt = m
    assert ip.dtype == np.dtype(ptr) and ix.dtype == np.dtype(idx)
    shape = (outer, inner) if storage == _ffi.CSR else (inner, outer)
    fresh_blocks()
    o = dev((shape, ip, ix, dt), storage=storage).to_other_storage()
    rip, rix, rdt = oracle.convert_storage(outer, inner, ip, ix, dt, mat_rows=shape[0])
    s2, gip, gix, gdt = o.to_host()
    assert tuple(s2) == shape and o.storage() == (_ffi.CSC if storage == _ffi.CSR else _ffi.CSR)
    assert gip.dtype == np.dtype(ptr) and gix.dtype == np.dtype(idx) and gip.size == inner + 1
    assert np.array_equal(gip, rip)
    assert np.array_equal(gix, rix)
    assert np.array_equal(gdt.view(np.uint64), rdt.view(np.uint64))
    fresh_blocks()
    back = o.to_other_storage()
    s3, bip, bix, bdt = back.to_host()
    assert tuple(s3) == shape and back.storage() == storage
    assert bip.dtype == ip.dtype and bix.dtype == ix.dtype
    assert np.array_equal(bip, ip) and np.array_equal(bix, ix) and np.array_equal(bdt.view(np.uint64), dt.view(np.uint64))
    return gip, gix, gdt


ROW_CLASSES = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 0, 1500, 0]


@pytest.mark.parametrize("idx,ptr", IDX_COMBOS)
def test_output_row_length_classes(hip, idx, ptr):
    """output rows of 0 / 1 entries (shortcuts), around the bitonic sort's power-of-two paddings, and on both sides of the
    1024-entry switch from the one-wave kernel to the workgroup kernel"""
    rng = np.random.default_rng(41)
    rows = 1600
    o = np.concatenate([rng.permutation(rows)[:k] for k in ROW_CLASSES])
    c = np.repeat(np.arange(len(ROW_CLASSES)), ROW_CLASSES)
    gip, gix, _ = check_conversion(csr_from_cells(rows, len(ROW_CLASSES), o, c, 42, idx, ptr), idx, ptr)
    assert np.diff(gip.astype(np.int64)).tolist() == ROW_CLASSES
    for j in range(len(ROW_CLASSES)):                          # independent of the oracle: every output row sorted, no entry lost
        assert np.array_equal(gix[int(gip[j]):int(gip[j + 1])], np.sort(o[c == j]).astype(idx))


@pytest.mark.parametrize("idx,ptr", IDX_COMBOS)
@pytest.mark.parametrize("shape", [(0, 5), (5, 0), (5, 7)])
def test_degenerate_shapes(hip, shape, idx, ptr):
    from sprs_amd import _ffi
    for storage in (_ffi.CSR, _ffi.CSC):
        outer, inner = shape if storage == _ffi.CSR else shape[::-1]
        fresh_blocks()
        o = dev((shape, np.zeros(outer + 1, dtype=ptr), np.zeros(0, dtype=idx), np.zeros(0)), storage=storage).to_other_storage()
        s2, gip, gix, gdt = o.to_host()
        assert tuple(s2) == shape and o.storage() == (_ffi.CSC if storage == _ffi.CSR else _ffi.CSR) and o.nnz() == 0
        assert gip.dtype == np.dtype(ptr) and gix.dtype == np.dtype(idx)
        assert gip.tolist() == [0] * (inner + 1) and gix.size == 0 and gdt.size == 0


def rows_over_inner(n_rows, inner, per_row, forced, seed):
    rng = np.random.default_rng(seed)
    o, c = [], []
    for r in range(n_rows):
        cols = rng.permutation(inner)[:per_row] if inner < 10000 else rng.integers(0, inner, per_row)
        cols = np.unique(np.concatenate([cols, forced if r in (0, n_rows - 1) else []]).astype(np.int64))
        o.append(np.full(cols.size, r))
        c.append(cols)
    return np.concatenate(o), np.concatenate(c)


@pytest.mark.parametrize("idx,ptr", IDX_COMBOS)
@pytest.mark.parametrize("inner", [255, 256, 257, 512, 2047, 2048, 2049, 4096, 4097])
def test_scan_seams_over_inner(hip, inner, idx, ptr):
    """the histogram is scanned over `inner`: one below, on and one above the scan's 256-thread and 2048-element tiles (and
    the 256-thread grids of the indptr kernels); the first and the last column are occupied"""
    n_rows = 3 + inner % 2
    o, c = rows_over_inner(n_rows, inner, min(inner, 300), [0, inner - 1], seed=inner)
    gip, _, _ = check_conversion(csr_from_cells(n_rows, inner, o, c, inner + 1, idx, ptr), idx, ptr)
    assert int(gip[1]) >= 2 and int(gip[-1]) - int(gip[-2]) >= 2 and int(gip[-1]) == o.size   # first and last row hold them


def test_scan_third_level_over_inner(hip):
    """inner = 2^21 + 4097 = 1027 scan tiles: scan_sums_kernel goes round its loop twice and carries the first 1024 block
    sums into the second round; entries on both sides of element 2^21"""
    inner = (1 << 21) + 4097
    forced = [0, (1 << 21) - 1, 1 << 21, (1 << 21) + 1, inner - 1]
    o, c = rows_over_inner(3, inner, 4000, forced, seed=5)
    gip, _, _ = check_conversion(csr_from_cells(3, inner, o, c, 6), np.uint64, np.uint64)
    for j in forced:
        assert int(gip[j + 1]) - int(gip[j]) >= 2              # rows 0 and 2 hold them
    assert int(gip[1 << 21]) > 0 and int(gip[-1]) == o.size


@pytest.mark.parametrize("idx,ptr", [(np.uint64, np.uint64), (np.uint32, np.uint32)])
def test_hub_column_over_three_bitmap_windows(hip, idx, ptr):
    """a column of ~350 k entries over 2 * 2^19 + 5000 rows: the workgroup kernel walks three 2^19-row bitmap windows, with
    entries on the last row of a window and the first two of the next; beside it a second long column and a short one"""
    w = 1 << 19
    rows = 2 * w + 5000
    c1 = np.unique(np.concatenate([np.arange(0, rows, 3), [w - 1, w, w + 1, 2 * w - 1, 2 * w, 2 * w + 1, rows - 1]]))
    c0 = np.arange(5, rows, 7)
    c2 = np.arange(0, rows, 1500)
    assert c0.size > 1024 and 1 < c2.size <= 1024
    o = np.concatenate([c0, c1, c2])
    c = np.repeat([0, 1, 2], [c0.size, c1.size, c2.size])
    gip, gix, _ = check_conversion(csr_from_cells(rows, 3, o, c, 8, idx, ptr), idx, ptr)
    assert gip.tolist() == [0, c0.size, c0.size + c1.size, o.size]
    assert np.array_equal(gix, np.concatenate([c0, c1, c2]).astype(idx))


def check_slice(m, d, storage, start, end):
    from sprs_amd import _ffi
    (outer, inner), ip, ix, dt = m
    fresh_blocks()
    s = d.slice_outer(start, end)
    shape, gip, gix, gdt = s.to_host()
    n = end - start
    lo, hi = int(ip[start]), int(ip[end])
    assert s.storage() == storage and tuple(shape) == ((n, inner) if storage == _ffi.CSR else (inner, n))
    assert gip.dtype == ip.dtype and gix.dtype == ix.dtype and gip.size == n + 1 and s.nnz() == hi - lo
    assert int(gip[0]) == 0 and np.array_equal(gip.astype(np.int64), ip[start:end + 1].astype(np.int64) - lo)
    assert np.array_equal(gix, ix[lo:hi]) and np.array_equal(gdt.view(np.uint64), dt[lo:hi].view(np.uint64))


@pytest.mark.parametrize("idx,ptr", IDX_COMBOS)
@pytest.mark.parametrize("k", [255, 256, 257, 512])
def test_slice_outer_seams(hip, k, idx, ptr):
    """slices of k outer slices: k + 1 indptr entries on both sides of the 256-thread grid of the rebase kernel"""
    from sprs_amd import _ffi
    outer, inner = k + 40, 50
    lens = np.random.default_rng(k).integers(0, 9, outer)
    lens[[7, 12, 20, outer - 1]] = 0                            # empty outer slices at the cuts below
    lens[[6, 8, 11, 13, 19, 21]] = 3
    m = ragged_csr(lens, inner, seed=k + 1, idx=idx, ptr=ptr, positive=False)
    for storage in (_ffi.CSR, _ffi.CSC):
        d = dev(((outer, inner) if storage == _ffi.CSR else (inner, outer),) + m[1:], storage=storage)
        for start, end in [(7, 7 + k), (0, outer), (0, k), (outer - k, outer), (k, k), (0, 0), (outer, outer),
                           (7, 13), (8, 12), (12, 20), (13, 21), (12, 13)]:
            check_slice(m, d, storage, start, end)
