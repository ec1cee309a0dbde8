"""Device sparse vectors and the CsMat x CsVec / CsVec x CsMat products (vec.rs:1084-1131, prod.rs:161-184), bit for bit.

The small cases (golden, order, errors, widths) also run against the kernel emulator (tests/test_csvec_emu_cpu.py); the torch
stream cases need a real device."""
import os

import numpy as np
import pytest

from conftest import as_csr
from csvec_ref import bits, csr_mul_csvec_ref, masked_dot_vec
from helpers import ragged_csr

pytestmark = pytest.mark.gpu

EMULATED = bool(os.environ.get("SPRS_HIP_LIBRARY"))


@pytest.fixture(scope="module", autouse=True)
def _need_device():
    import sprs_amd
    if sprs_amd.device_count() < 1:
        pytest.skip("no HIP device")


def _mat(shape, ip, ix, dt, storage=0):
    from sprs_amd.device import DeviceCsMat
    return DeviceCsMat.from_host(shape, ip, ix, dt, storage=storage)


def _vec(dim, idx, val, dtype=np.uint64):
    from sprs_amd.device import DeviceCsVec
    return DeviceCsVec.from_host(dim, np.asarray(idx, dtype=dtype), np.asarray(val, dtype=np.float64))


def _same(res, dim, idx, val):
    d, i, v = res.to_host()
    assert d == dim
    assert np.array_equal(i.astype(np.int64), np.asarray(idx, dtype=np.int64)), (i, idx)
    assert np.array_equal(bits(v), bits(val)), (v, val)


def _ragged(rows, cols, seed):
    """rows of 0 to 60 entries and a few of up to 3 x CV_LONG (whole-wave slices), signed values"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 60, rows)
    lens[rng.choice(rows, max(1, rows // 50), replace=False)] = rng.integers(100, min(cols, 400), max(1, rows // 50))
    return ragged_csr(lens, cols, seed=seed, positive=False)


def _to_csc(shape, ip, ix, dt):
    """the CSC arrays of a CSR matrix (stable: column entries by ascending row)"""
    rows, cols = shape
    ip = np.asarray(ip, dtype=np.int64)
    row_of = np.repeat(np.arange(rows), np.diff(ip))
    order = np.lexsort((row_of, np.asarray(ix, dtype=np.int64)))
    cip = np.zeros(cols + 1, dtype=np.int64)
    np.add.at(cip, np.asarray(ix, dtype=np.int64) + 1, 1)
    return np.cumsum(cip).astype(np.uint64), row_of[order].astype(np.uint64), np.asarray(dt)[order]


# ---- the reference's own tests (prod.rs:461-500) ----------------------------------------------------------------------------

V5 = (5, [0, 2, 4], [1.0, 1.0, 1.0])


def test_golden_mul_csr_csvec(golden):
    """prod.rs:461-468 mul_csr_csvec: expected CsVec::new(5, [0, 1, 2], [3, 5, 5])"""
    a = _mat(*as_csr(golden["mat1"]))
    _same(a * _vec(*V5), 5, [0, 1, 2], [3.0, 5.0, 5.0])


def test_golden_mul_csr_zero_csvec(golden):
    """prod.rs:470-474 mul_csr_zero_csvec: &mat1() * &CsVec::new(0, [], []) == that empty vector (dimension 0)"""
    a = _mat(*as_csr(golden["mat1"]))
    _same(a * _vec(0, [], []), 0, [], [])


def test_golden_mul_csvec_csr(golden):
    """prod.rs:476-483 mul_csvec_csr: expected CsVec::new(5, [2, 3], [8, 11])"""
    a = _mat(*as_csr(golden["mat1"]))
    _same(_vec(*V5) * a, 5, [2, 3], [8.0, 11.0])


def test_golden_mul_csc_csvec(golden):
    """prod.rs:485-491 mul_csc_csvec: expected CsVec::new(5, [0, 1, 2], [3, 5, 5])"""
    a = _mat(*as_csr(golden["mat1_csc"]), storage=1)
    _same(a * _vec(*V5), 5, [0, 1, 2], [3.0, 5.0, 5.0])


def test_golden_mul_csvec_csc(golden):
    """prod.rs:493-500 mul_csvec_csc: expected CsVec::new(5, [2, 3], [8, 11])"""
    a = _mat(*as_csr(golden["mat1_csc"]), storage=1)
    _same(_vec(*V5) * a, 5, [2, 3], [8.0, 11.0])


# ---- order sensitivity, signed zeros, explicit zeros, NaN / inf -------------------------------------------------------------

def _order_case():
    """rows whose ordered sum is exactly 0 only in sprs' order, a single -0.0 product, explicit zeros, NaN, inf"""
    inf, nan = float("inf"), float("nan")
    rows = [
        ([0, 1, 2, 3], [1e16, 1.0, -1e16, -1.0]),     # cancellations of 1e16: the result depends on the order
        ([0, 2, 1 + 2, 4], [1.0, 1e16, -1e16, -1.0]),  # (1 + 1e16 - 1e16) + (-5) in order; 0 - 5 in another
        ([1], [-1.0]),                                  # times v[1] = +0.0: the single product is -0.0
        ([4], [0.0]),                                   # explicit zero in A
        ([5], [2.0]),                                   # times the explicit zero of v
        ([0, 6], [1.0, inf]),                           # inf
        ([7], [nan]),                                   # NaN is != 0: kept by csr_mul_csvec
        ([8], [3.0]),                                   # no match
        ([], []),                                       # empty row
        ([0, 3], [1.0, 1.0]),                           # 1 + (-1) = 0 exactly: dropped by CSR, stored by the others
        ([2, 3, 6], [1e-300, 1e-300, -inf]),
    ]
    ip = np.cumsum([0] + [len(r[0]) for r in rows]).astype(np.uint64)
    ix = np.concatenate([np.array(r[0], dtype=np.uint64) for r in rows])
    dt = np.concatenate([np.array(r[1], dtype=np.float64) for r in rows])
    shape = (len(rows), 9)
    vidx = np.array([0, 1, 2, 3, 4, 5, 6, 7], dtype=np.uint64)
    vval = np.array([1.0, 0.0, 1.0, -1.0, 5.0, 0.0, 2.0, 1.0])
    return shape, ip, ix, dt, vidx, vval


def test_order_of_additions_csr():
    shape, ip, ix, dt, vidx, vval = _order_case()
    d, ei, ed = csr_mul_csvec_ref(ip, ix, dt, shape[0], shape[1], vidx, vval)
    assert 2 not in ei and 9 not in ei and 6 in ei        # the -0.0 row and the exact cancellation dropped, NaN kept
    res = _mat(shape, ip, ix, dt) * _vec(shape[1], vidx, vval)
    _same(res, d, ei, ed)


def test_order_of_additions_structural():
    from oracle import oracle
    shape, ip, ix, dt, vidx, vval = _order_case()
    d, ei, ed = csr_mul_csvec_ref(ip, ix, dt, shape[0], shape[1], vidx, vval, structural=True)
    # sprs' own route for CSC A x v: mul_csr_csr of A (CSR form) with v as an n x 1 matrix
    v_ip = np.searchsorted(vidx, np.arange(shape[1] + 1)).astype(np.uint64)
    _, rip, rix, rdt = oracle.mul_csr_csr(shape, ip, ix, dt, (shape[1], 1), v_ip, np.zeros(vidx.size, dtype=np.uint64), vval, threads=1)
    nz_rows = np.nonzero(np.diff(rip.astype(np.int64)))[0]
    assert np.array_equal(nz_rows, ei) and np.array_equal(bits(rdt), bits(ed))
    # CSC A x v
    cip, cix, cdt = _to_csc(shape, ip, ix, dt)
    a_csc = _mat(shape, cip, cix, cdt, storage=1)
    _same(a_csc * _vec(shape[1], vidx, vval), d, ei, ed)
    # v x B with B = A^T: column o of B is row o of A
    b_csr = _mat((shape[1], shape[0]), cip, cix, cdt, storage=0)
    b_csc = _mat((shape[1], shape[0]), ip, ix, dt, storage=1)
    _same(_vec(shape[1], vidx, vval) * b_csr, d, ei, ed)
    _same(_vec(shape[1], vidx, vval) * b_csc, d, ei, ed)


def test_signed_zero_results():
    """one -0.0 product: dropped by csr_mul_csvec (0.0 + -0.0 = +0.0 == 0), stored as +0.0 by the structural routes"""
    ip = np.array([0, 1], dtype=np.uint64)
    ix = np.array([0], dtype=np.uint64)
    dt = np.array([-1.0])
    v = _vec(1, [0], [0.0])
    _same(_mat((1, 1), ip, ix, dt) * v, 1, [], [])
    res = _mat((1, 1), ip, ix, dt, storage=1) * v
    _same(res, 1, [0], [0.0])
    assert np.signbit(res.to_host()[2][0]) == False   # noqa: E712


# ---- index widths -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("widths", [(8, 8, 8), (4, 4, 4), (4, 8, 4), (8, 4, 8), (2, 2, 2), (4, 4, 2), (8, 8, 4)])
def test_index_widths(widths):
    ipw, ixw, vw = widths
    dtp = {2: np.uint16, 4: np.uint32, 8: np.uint64}
    shape, ip, ix, dt = _ragged(300, 500, 3)
    ip, ix = ip.astype(dtp[ipw]), ix.astype(dtp[ixw])
    rng = np.random.default_rng(5)
    vidx = np.sort(rng.choice(500, 120, replace=False))
    vval = rng.standard_normal(120)
    v = _vec(500, vidx, vval, dtype=dtp[vw])
    d, ei, ed, _ = masked_dot_vec(ip, ix, dt, 300, 500, vidx, vval)
    res = _mat(shape, ip, ix, dt) * v
    _same(res, d, ei, ed)
    assert res.index_bytes() == ixw and res.to_host()[1].dtype == dtp[ixw]
    d, ei, ed, _ = masked_dot_vec(ip, ix, dt, 300, 500, vidx, vval, structural=True)
    cip, cix, cdt = _to_csc(shape, ip, ix, dt)
    _same(v * _mat((500, 300), cip.astype(dtp[ipw]), cix.astype(dtp[ixw]), cdt), d, ei, ed)


def test_result_index_overflow():
    """a u16 CSR matrix with 70000 rows is valid (the index type bounds the columns); a kept row >= 65536 cannot be stored
    (I::from_usize in CsVec::append panics)"""
    from sprs_amd import SprsHipError, _ffi
    rows = 70000
    ip = np.zeros(rows + 1, dtype=np.uint32)
    ip[-1] = 1
    ix = np.array([3], dtype=np.uint16)
    a = _mat((rows, 4), ip, ix, np.array([2.0]))
    with pytest.raises(SprsHipError) as e:
        a * _vec(4, [3], [1.0], dtype=np.uint16)
    assert e.value.status == _ffi.INDEX_OVERFLOW
    ip2 = np.zeros(rows + 1, dtype=np.uint32)
    ip2[1:] = 1
    _same(_mat((rows, 4), ip2, ix, np.array([2.0])) * _vec(4, [3], [1.0], dtype=np.uint16), rows, [0], [2.0])


# ---- errors -------------------------------------------------------------------------------------------------------------------

def test_upload_errors():
    from sprs_amd import SprsHipError, _ffi
    from sprs_amd.device import DeviceCsVec
    cases = [
        ((5, np.array([2, 1], dtype=np.uint64), [1.0, 1.0]), _ffi.BAD_STRUCTURE, "Unsorted indices"),
        ((5, np.array([1, 1], dtype=np.uint64), [1.0, 1.0]), _ffi.BAD_STRUCTURE, "Unsorted indices"),
        ((5, np.array([1, 5], dtype=np.uint64), [1.0, 1.0]), _ffi.BAD_STRUCTURE, "indices larger than vector size"),
        ((5, np.array([1, 2], dtype=np.uint64), [1.0]), _ffi.BAD_STRUCTURE, "indices and data do not have compatible lengths"),
        ((70000, np.array([1], dtype=np.uint16), [1.0]), _ffi.INDEX_OVERFLOW, "Index size is too small"),
    ]
    for (dim, idx, val), status, text in cases:
        with pytest.raises(SprsHipError) as e:
            DeviceCsVec.from_host(dim, idx, np.asarray(val))
        assert e.value.status == status and text in str(e.value), str(e.value)
    # trusted: no check
    assert DeviceCsVec.from_host(5, np.array([2, 1], dtype=np.uint64), np.ones(2), validate=False).nnz() == 2


def test_upload_errors_checked_on_the_device():
    """vectors above the host-check size are validated by csvec_check_kernel"""
    from sprs_amd import SprsHipError, _ffi
    from sprs_amd.device import DeviceCsVec
    n = (1 << 16) + 100
    idx = np.arange(n, dtype=np.uint64) * 2
    assert DeviceCsVec.from_host(2 * n, idx, np.ones(n)).nnz() == n
    bad = idx.copy()
    bad[60000], bad[60001] = bad[60001], bad[60000]
    with pytest.raises(SprsHipError) as e:
        DeviceCsVec.from_host(2 * n, bad, np.ones(n))
    assert e.value.status == _ffi.BAD_STRUCTURE and "Unsorted indices" in str(e.value)
    with pytest.raises(SprsHipError) as e:
        DeviceCsVec.from_host(2 * n - 2, idx, np.ones(n))
    assert e.value.status == _ffi.BAD_STRUCTURE and "indices larger than vector size" in str(e.value)


def test_dimension_errors(golden):
    from sprs_amd import SprsHipError, _ffi, prod
    a = _mat(*as_csr(golden["mat1"]))
    a_csc = _mat(*as_csr(golden["mat1_csc"]), storage=1)
    for lhs, rhs in ((a, _vec(4, [0], [1.0])), (a_csc, _vec(6, [0], [1.0])), (_vec(4, [0], [1.0]), a), (_vec(6, [0], [1.0]), a_csc),
                     (a_csc, _vec(0, [], [])), (_vec(0, [], []), a)):
        with pytest.raises(SprsHipError) as e:
            lhs * rhs
        assert e.value.status == _ffi.DIM_MISMATCH and str(e.value).endswith("Dimension mismatch")
    with pytest.raises(SprsHipError) as e:
        prod.csr_mul_csvec(a_csc, _vec(5, [0], [1.0]))
    assert e.value.status == _ffi.STORAGE_MISMATCH
    _same(prod.csr_mul_csvec(a, _vec(*V5)), 5, [0, 1, 2], [3.0, 5.0, 5.0])


def test_empty_operands():
    ip = np.array([0, 1, 1, 3], dtype=np.uint64)
    ix = np.array([2, 0, 1], dtype=np.uint64)
    dt = np.array([1.0, 2.0, 3.0])
    a = _mat((3, 4), ip, ix, dt)
    _same(a * _vec(4, [], []), 3, [], [])
    _same(_mat((3, 4), *_to_csc((3, 4), ip, ix, dt), storage=1) * _vec(4, [], []), 3, [], [])
    _same(_vec(3, [], []) * a, 4, [], [])
    z = _mat((0, 4), np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint64), np.zeros(0))
    _same(z * _vec(4, [1], [1.0]), 0, [], [])
    z2 = _mat((3, 0), np.zeros(4, dtype=np.uint64), np.zeros(0, dtype=np.uint64), np.zeros(0))
    _same(z2 * _vec(0, [], []), 0, [], [])          # dim 0: CsVecI::empty(0)
    _same(_vec(3, [0], [1.0]) * z2, 0, [], [])


def test_small_ragged_all_densities():
    """ragged rows (some longer than the one-lane-per-slice limit), densities from one entry to all of v"""
    shape, ip, ix, dt = _ragged(700, 900, 11)
    ip = ip.astype(np.uint64)
    rng = np.random.default_rng(2)
    a = _mat(shape, ip, ix, dt)
    cip, cix, cdt = _to_csc(shape, ip, ix, dt)
    a_csc = _mat(shape, cip, cix, cdt, storage=1)
    for k in (1, 9, 90, 450, 900):
        vidx = np.sort(rng.choice(900, k, replace=False))
        vval = rng.standard_normal(k)
        v = _vec(900, vidx, vval)
        d, ei, ed, _ = masked_dot_vec(ip, ix, dt, 700, 900, vidx, vval)
        _same(a * v, d, ei, ed)
        d, ei, ed, _ = masked_dot_vec(ip, ix, dt, 700, 900, vidx, vval, structural=True)
        _same(a_csc * v, d, ei, ed)


def test_hub_rows_small():
    """rows of several thousand entries next to short ones: the whole-wave path and the segments around it"""
    rng = np.random.default_rng(4)
    lens = rng.integers(0, 40, 300)
    lens[[3, 64, 65, 200, 299]] = [5000, 3000, 700, 129, 4000]
    n = 6000
    ip = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    ix = np.concatenate([np.sort(rng.choice(n, int(l), replace=False)) for l in lens]).astype(np.uint64)
    dt = rng.standard_normal(ix.size)
    dt[rng.random(ix.size) < 0.01] = 0.0
    a = _mat((300, n), ip, ix, dt)
    for dens in (0.001, 0.3, 1.0):
        k = max(1, int(n * dens))
        vidx = np.sort(rng.choice(n, k, replace=False))
        vval = rng.standard_normal(k)
        d, ei, ed, _ = masked_dot_vec(ip, ix, dt, 300, n, vidx, vval)
        _same(a * _vec(n, vidx, vval), d, ei, ed)


def test_cross_check_with_spgemm():
    """CSC x v and v x CSR / CSC give the bits of sprs_hip_csmat_mul_csmat with the vector wrapped as a matrix"""
    from sprs_amd.device import DeviceCsMat
    shape, ip, ix, dt = _ragged(400, 600, 21)
    ip = ip.astype(np.uint64)
    rng = np.random.default_rng(8)
    vidx = np.sort(rng.choice(600, 200, replace=False)).astype(np.uint64)
    vval = rng.standard_normal(200)
    v = _vec(600, vidx, vval)
    cip, cix, cdt = _to_csc(shape, ip, ix, dt)
    a_csc = DeviceCsMat.from_host(shape, cip, cix, cdt, storage=1)
    col = DeviceCsMat.from_host((600, 1), np.array([0, 200], dtype=np.uint64), vidx, vval, storage=1)   # v.col_view()
    m = (a_csc * col).to_host()          # CSC result (400 x 1): column 0
    _, mip, mix, mdt = m
    _same(a_csc * v, 400, mix, mdt)
    b = DeviceCsMat.from_host((600, 400), cip, cix, cdt)   # A^T as CSR
    row = DeviceCsMat.from_host((1, 600), np.array([0, 200], dtype=np.uint64), vidx, vval)
    _, rip, rix, rdt = (row * b).to_host()
    _same(v * b, 400, rix, rdt)
    _same(v * DeviceCsMat.from_host((600, 400), ip, ix, dt, storage=1), 400, rix, rdt)


def test_scatter_to_dense():
    from sprs_amd.device import DeviceVec
    rng = np.random.default_rng(1)
    vidx = np.sort(rng.choice(1000, 77, replace=False))
    vval = rng.standard_normal(77)
    v = _vec(1000, vidx, vval, dtype=np.uint32)
    want = np.zeros(1000)
    want[vidx] = vval
    assert np.array_equal(v.to_dense().to_host(), want)
    out = DeviceVec.from_host(np.full(1000, 7.0))
    assert np.array_equal(v.scatter(out).to_host(), want)
    from sprs_amd import SprsHipError
    with pytest.raises(SprsHipError):
        v.scatter(DeviceVec(999))


# ---- scale (real device only) --------------------------------------------------------------------------------------------------

@pytest.mark.skipif(EMULATED, reason="large operands: real device only")
def test_rmat_1m_all_operators():
    from sprs_amd import gen
    n = 1 << 20
    indptr, indices, data = gen.rmat_csr(n, 16, seed=3)
    ip = indptr.numpy().astype(np.uint64)
    ix = indices.numpy().astype(np.uint64)
    dt = data.numpy()
    a = _mat((n, n), ip, ix, dt)
    cip, cix, cdt = _to_csc((n, n), ip, ix, dt)
    a_csc = _mat((n, n), cip, cix, cdt, storage=1)
    assert int(np.diff(ip.astype(np.int64)).max()) >= 10 ** 4
    rng = np.random.default_rng(6)
    for k in (1, 100, 10000, n // 10, n):
        vidx = np.sort(rng.choice(n, k, replace=False)) if k < n else np.arange(n)
        vval = rng.standard_normal(k)
        v = _vec(n, vidx, vval)
        d, ei, ed, _ = masked_dot_vec(ip, ix, dt, n, n, vidx, vval)
        _same(a * v, d, ei, ed)
        d, ei, ed, _ = masked_dot_vec(ip, ix, dt, n, n, vidx, vval, structural=True)
        _same(a_csc * v, d, ei, ed)
        if k in (100, n):
            dt_, et, edt, _ = masked_dot_vec(cip, cix, cdt, n, n, vidx, vval, structural=True)
            _same(v * a, dt_, et, edt)          # v x CSR: columns of A, i.e. rows of the CSC form
            _same(v * a_csc, dt_, et, edt)


@pytest.mark.skipif(EMULATED, reason="large operands: real device only")
def test_ragged_hub_rows_1e5():
    rng = np.random.default_rng(12)
    rows, n = 5000, 400000
    lens = rng.integers(0, 60, rows)
    lens[[0, 777, 4999]] = [150000, 100000, 120000]
    ip = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    ix = np.concatenate([np.sort(rng.choice(n, int(l), replace=False)) for l in lens]).astype(np.uint32)
    dt = rng.standard_normal(ix.size)
    a = _mat((rows, n), ip, ix, dt)
    for k in (3, 4000, n):
        vidx = np.sort(rng.choice(n, k, replace=False)) if k < n else np.arange(n)
        vval = rng.standard_normal(k)
        d, ei, ed, _ = masked_dot_vec(ip, ix, dt, rows, n, vidx, vval)
        _same(a * _vec(n, vidx, vval, dtype=np.uint32), d, ei, ed)


# ---- streams and borrowed memory (torch) -----------------------------------------------------------------------------------------

@pytest.mark.skipif(EMULATED, reason="torch streams: real device only")
def test_non_blocking_stream_and_borrow():
    """the vector is written on a non-blocking torch stream and multiplied there with no host synchronise in between: the
    product's read-back of nnz is ordered on that stream"""
    import torch
    from sprs_amd import prod
    from sprs_amd.device import DeviceCsVec
    shape, ip, ix, dt = _ragged(2000, 3000, 5)
    ip = ip.astype(np.uint64)
    a = _mat(shape, ip, ix, dt)
    rng = np.random.default_rng(9)
    vidx = np.sort(rng.choice(3000, 1500, replace=False))
    vval = rng.standard_normal(1500)
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        ti = torch.zeros(1500, dtype=torch.int64, device=dev)
        td = torch.zeros(1500, dtype=torch.float64, device=dev)
        torch.cuda._sleep(20_000_000)                  # keep the stream busy: the copies below land late
        ti.copy_(torch.from_numpy(vidx.astype(np.int64)).to(dev, non_blocking=True))
        td.copy_(torch.from_numpy(vval).to(dev, non_blocking=True))
        v = DeviceCsVec.borrow(3000, ti, td)
        res = prod.csmat_mul_csvec(a, v, stream=s)
    d, ei, ed, _ = masked_dot_vec(ip, ix, dt, 2000, 3000, vidx, vval)
    _same(res, d, ei, ed)
    ti32 = torch.from_numpy(vidx.astype(np.int32)).to(dev)
    v32 = DeviceCsVec.borrow(3000, ti32, torch.from_numpy(vval).to(dev))
    torch.cuda.synchronize()
    _same(a * v32, d, ei, ed)
    out = torch.full((3000,), 5.0, dtype=torch.float64, device=dev)
    from sprs_amd.device import DeviceVec
    v32.scatter(DeviceVec.borrow(out))
    want = np.zeros(3000)
    want[vidx] = vval
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
