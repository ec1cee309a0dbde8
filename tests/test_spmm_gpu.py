"""GPU parity tests of the SpMM path (prod::csr_mulacc_dense_rowmaj twin, prod.rs:189-214) against
the reference's golden vectors and the oracle (SpMM == SpMV per rhs column, prod.rs:274-298)."""
import numpy as np
import pytest

from conftest import IDX_COMBOS, as_csr
from helpers import fresh_blocks, ragged_csr, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-10


@pytest.fixture(scope="module")
def hip():
    import sprs_amd
    if sprs_amd.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X (no CPU fallback exists)")
    return sprs_amd


def oracle_spmm(shape, ip, ix, dt, rhs, out0=None):
    from oracle import oracle
    out = np.zeros((shape[0], rhs.shape[1])) if out0 is None else out0.copy()
    for j in range(rhs.shape[1]):
        col = np.ascontiguousarray(out[:, j])
        oracle.mul_acc_mat_vec_csr(shape, ip, ix, dt, np.ascontiguousarray(rhs[:, j]), col)
        out[:, j] = col
    return out


@pytest.mark.parametrize("idx,ptr", IDX_COMBOS)
def test_golden_mul_csr_dense_rowmaj(hip, golden, idx, ptr):
    # prod.rs:502-542: eye(3) * eye(3); mat1 * mat_dense1 (exact); mat5 * mat_dense2 (eps 1e-8)
    from sprs_amd import prod
    from sprs_amd.device import DeviceCsMat
    e = DeviceCsMat.eye(3)
    a = prod.DeviceMat.from_host(np.eye(3))
    res = prod.DeviceMat(3, 3)
    prod.csr_mulacc_dense_rowmaj(e, a, res)
    assert np.array_equal(res.to_host(), np.eye(3))
    for mk, dk, ek in (("mat1", "mat_dense1", "mat1_times_mat_dense1"), ("mat5", "mat_dense2", "mat5_times_mat_dense2")):
        m = DeviceCsMat.from_host(*as_csr(golden[mk], idx, ptr))
        b = prod.DeviceMat.from_host(np.array(golden[dk]))
        exp = np.array(golden[ek]["rows"])
        res = prod.DeviceMat(exp.shape[0], exp.shape[1])
        prod.csr_mulacc_dense_rowmaj(m, b, res)
        assert np.all(np.abs(res.to_host() - exp) <= golden[ek]["epsilon"])
        c = (m * b).to_host()                                  # `&a * &b` (csmat.rs:1989-2048)
        assert np.all(np.abs(c - exp) <= golden[ek]["epsilon"])
        prod.csr_mulacc_dense_rowmaj(m, b, res)                # accumulates
        assert np.all(np.abs(res.to_host() - 2 * exp) <= 2 * golden[ek]["epsilon"] + 1e-12)


def test_golden_mul_csc_dense(hip, golden):
    """prod.rs:545-597: mul_csc_dense_rowmaj, mul_csc_dense_colmaj, mul_csr_dense_colmaj — mat1 (CSC / CSR) * mat_dense1 in both
    layouts, the explicit kernels and `&a * &b`; and the (CSC, cols < 8) / (CSC, cols >= 8) arms of the dispatch on wider data"""
    from sprs_amd import prod
    from sprs_amd.device import DeviceCsMat, DeviceVec, CSC
    exp = np.array(golden["mat1_times_mat_dense1"]["rows"])
    dense = np.array(golden["mat_dense1"])
    g = golden["mat1_csc"]
    u = lambda v: np.array(v, dtype=np.uint64)
    a_csc = DeviceCsMat.from_host(tuple(g["shape"]), u(g["indptr"]), u(g["indices"]), np.array(g["data"]), storage=CSC)
    a_csr = DeviceCsMat.from_host(*as_csr(golden["mat1"], np.uint64, np.uint64))
    b = prod.DeviceMat.from_host(dense)
    res = prod.DeviceMat(5, 5)
    prod.csc_mulacc_dense_rowmaj(a_csc, b, res)                           # mul_csc_dense_rowmaj
    assert np.array_equal(res.to_host(), exp)
    assert np.array_equal((a_csc * b).to_host(), exp)
    for a, kernel in ((a_csc, prod.csc_mulacc_dense_colmaj), (a_csr, prod.csr_mulacc_dense_colmaj)):   # the two colmaj tests
        cols_in = [DeviceVec.from_host(np.ascontiguousarray(dense[:, j])) for j in range(5)]
        cols_out = [DeviceVec.zeros(5) for _ in range(5)]
        kernel(a, cols_in, cols_out)
        assert np.array_equal(np.stack([c.to_host() for c in cols_out], axis=1), exp)
    with pytest.raises(hip.SprsHipError) as e:                            # assert!(lhs.is_csc(), "Storage mismatch")
        prod.csc_mulacc_dense_rowmaj(a_csr, b, res)
    assert e.value.status == hip._ffi.STORAGE_MISMATCH
    with pytest.raises(hip.SprsHipError) as e:
        prod.csc_mulacc_dense_rowmaj(a_csc, prod.DeviceMat(4, 5), res)
    assert e.value.status == hip._ffi.DIM_MISMATCH
    # wider: a random CSC matrix times 3 and 11 columns against the oracle on its CSR form
    import scipy.sparse as sp
    rng = np.random.default_rng(8)
    m = sp.random(300, 200, density=0.05, random_state=4, format="csc")
    m.sort_indices()
    d = DeviceCsMat.from_host((300, 200), u(m.indptr), u(m.indices), m.data, storage=CSC)
    mr = m.tocsr()
    mr.sort_indices()
    for k in (3, 11):
        rhs = rng.standard_normal((200, k))
        got = (d * prod.DeviceMat.from_host(rhs)).to_host()
        ref = oracle_spmm((300, 200), u(mr.indptr), u(mr.indices), mr.data, rhs)
        assert rel_err(got, ref) <= 1e-10


@pytest.fixture(params=[(0, 1, 2), (0, 1, 1), (0, 0, 2), (2048, 1, 2)], ids=["stream", "stream-relaid-rhs", "chunks", "entry-order"])
def long_row(request, hip):
    """the summation modes of spmm.hip: tiles of 256 consecutive entries per wave (default) — gathering from the rhs itself or
    from its re-laid-out copy (option spmm_relayout) —, every row by 512-entry chunks (option spmm_stream = 0: the kernel of
    rounds 1-3), or rows of <= L entries in the reference's own entry order (option spmm_long_row = L: bit-identical to
    prod.rs:203-210)"""
    hip.set_option("spmm_long_row", request.param[0])
    hip.set_option("spmm_stream", request.param[1])
    hip.set_option("spmm_relayout", request.param[2])
    yield request.param[0]
    hip.set_option("spmm_long_row", -1)
    hip.set_option("spmm_stream", 1)
    hip.set_option("spmm_relayout", 0)


@pytest.mark.parametrize("k", [1, 3, 8, 16, 33, 64, 100])
def test_rmat_vs_oracle(hip, k, long_row):
    from sprs_amd import gen, prod
    from sprs_amd.device import DeviceCsMat
    n = 30000
    indptr, indices, data = gen.rmat_csr(n, 10, seed=13)        # rows longer than one 512-entry chunk too
    ip, ix, dt = indptr.numpy().astype(np.uint64), indices.numpy().astype(np.uint64), data.numpy()
    assert int(np.diff(ip.astype(np.int64)).max()) > 1500
    rng = np.random.default_rng(k)
    rhs = rng.random((n, k)) + 0.5
    a = DeviceCsMat.from_host((n, n), ip, ix, dt)
    got = (a * prod.DeviceMat.from_host(rhs)).to_host()
    ref = oracle_spmm((n, n), ip, ix, dt, rhs)
    assert rel_err(got, ref) <= TOL
    lens = np.diff(ip.astype(np.int64))
    short = (lens <= long_row) | (lens <= 1)                    # rows of <= L entries are summed in entry order, the
    assert np.array_equal(got[short], ref[short])               # reference's own (prod.rs:203-210): bit for bit
    empty = np.diff(ip.astype(np.int64)) == 0
    assert empty.any() and np.all(got[empty] == 0.0)
    out0 = rng.random((n, k))
    res = prod.DeviceMat.from_host(out0)
    prod.csr_mulacc_dense_rowmaj(a, prod.DeviceMat.from_host(rhs), res)
    got2 = res.to_host()
    ref2 = oracle_spmm((n, n), ip, ix, dt, rhs, out0)
    assert rel_err(got2, ref2) <= TOL
    assert np.array_equal(got2[short], ref2[short])             # the accumulate form starts from out[i, j], as there
    assert np.array_equal(got2[empty], out0[empty])             # empty rows untouched
    again = (a * prod.DeviceMat.from_host(rhs)).to_host()
    assert np.array_equal(got, again)                           # deterministic


@pytest.mark.parametrize("k", [2, 16, 40])
def test_long_rows_take_the_chunk_kernels(hip, k, long_row):
    """rows above option spmm_long_row are cut into 512-entry chunks (or, in the stream mode, cross several 256-entry tiles):
    same values up to the summation order"""
    from sprs_amd import prod
    from sprs_amd.device import DeviceCsMat
    rng = np.random.default_rng(100 + k)
    n, m = 300, 9000
    lens = rng.integers(0, 40, n)
    lens[[3, 150, 299]] = [2049, 7000, 4096]
    lens[[4, 151]] = [2048, 0]
    ip = np.zeros(n + 1, np.uint64)
    ip[1:] = np.cumsum(lens)
    ix = np.concatenate([np.sort(rng.choice(m, int(l), replace=False)) for l in lens]).astype(np.uint64)
    dt = rng.standard_normal(ix.size)
    rhs = rng.standard_normal((m, k))
    a = DeviceCsMat.from_host((n, m), ip, ix, dt)
    got = (a * prod.DeviceMat.from_host(rhs)).to_host()
    ref = oracle_spmm((n, m), ip, ix, dt, rhs)
    scale = np.abs(ref).max()
    assert np.abs(got - ref).max() <= 1e-12 * scale
    assert np.array_equal(got[lens <= max(long_row, 1)], ref[lens <= max(long_row, 1)])
    out0 = rng.standard_normal((n, k))
    res = prod.DeviceMat.from_host(out0)
    prod.csr_mulacc_dense_rowmaj(a, prod.DeviceMat.from_host(rhs), res)
    ref2 = oracle_spmm((n, m), ip, ix, dt, rhs, out0)
    assert np.abs(res.to_host() - ref2).max() <= 1e-12 * scale
    assert np.array_equal(res.to_host()[lens == 0], out0[lens == 0])


@pytest.mark.parametrize("k", [1, 5, 8, 16, 24, 64, 70])
@pytest.mark.parametrize("idx,ptr", IDX_COMBOS[:2])
def test_stream_tiles_and_runs(hip, k, idx, ptr):
    """the entry-stream kernel at its seams: rows that start exactly at a tile (256 entries) or run (256 / G) boundary, rows that
    cover several whole tiles, a row that begins in one tile's last entry, runs of empty rows across tile boundaries and at both
    ends, a last tile with a handful of entries; the accumulate form; strided (column-major) operands"""
    from sprs_amd import prod
    from sprs_amd.device import DeviceCsMat
    rng = np.random.default_rng(7 * k + np.dtype(idx).itemsize)
    lens = [0, 0, 256, 0, 32, 32, 64, 127, 1, 0, 0, 0, 255, 1, 256 * 3, 31, 1, 1000, 24, 0, 8, 8, 8, 8, 200, 56, 255, 257, 0, 0, 3]
    lens += [int(v) for v in rng.integers(0, 70, 400)] + [0] * 70 + [513, 0, 0]
    lens = np.array(lens)
    n, m = lens.size, 1500
    ip = np.zeros(n + 1, ptr)
    ip[1:] = np.cumsum(lens)
    ix = np.concatenate([np.sort(rng.choice(m, int(l), replace=False)) for l in lens]).astype(idx)
    dt = rng.standard_normal(ix.size)
    rhs = rng.standard_normal((m, k))
    a = DeviceCsMat.from_host((n, m), ip, ix, dt)
    ref = oracle_spmm((n, m), ip, ix, dt, rhs)
    bound = oracle_spmm((n, m), ip, ix, np.abs(dt), np.abs(rhs))
    for relayout in (2, 1):                                       # from the rhs itself, from its re-laid-out copy: the same bits
        hip.set_option("spmm_relayout", relayout)
        try:
            for col_major in (False, True):
                got = (a * prod.DeviceMat.from_host(rhs, col_major=col_major)).to_host()
                assert np.all(np.abs(got - ref) <= 64 * np.finfo(float).eps * bound)
                assert np.all(got[lens == 0] == 0.0)
                assert np.array_equal(got[lens == 1], ref[lens == 1])
                if relayout == 2 and not col_major:
                    plain = got
                elif not col_major:
                    assert np.array_equal(got, plain)
        finally:
            hip.set_option("spmm_relayout", 0)
    out0 = rng.standard_normal((n, k))
    ref2 = oracle_spmm((n, m), ip, ix, dt, rhs, out0)
    for col_major in (False, True):
        res = prod.DeviceMat.from_host(out0, col_major=col_major)
        kern = prod.csr_mulacc_dense_colmaj if col_major else prod.csr_mulacc_dense_rowmaj
        kern(a, prod.DeviceMat.from_host(rhs), res)
        assert np.all(np.abs(res.to_host() - ref2) <= 64 * np.finfo(float).eps * (np.abs(out0) + bound))
        assert np.array_equal(res.to_host()[lens == 0], out0[lens == 0])
    hip.set_option("spmm_stream", 0)                              # the chunk kernels agree to the summation order
    try:
        other = (a * prod.DeviceMat.from_host(rhs)).to_host()
    finally:
        hip.set_option("spmm_stream", 1)
    assert np.all(np.abs(other - ref) <= 64 * np.finfo(float).eps * bound)


def test_ragged_and_contract(hip, golden):
    from sprs_amd import SprsHipError, _ffi, prod
    from sprs_amd.device import DeviceCsMat
    lens = [0, 511, 512, 513, 0, 1, 2000, 3, 0]
    shape, ip, ix, dt = ragged_csr(lens, 5000, seed=2, positive=False)
    rng = np.random.default_rng(0)
    rhs = rng.standard_normal((5000, 12))
    a = DeviceCsMat.from_host(shape, ip, ix, dt)
    got = (a * prod.DeviceMat.from_host(rhs)).to_host()
    ref = oracle_spmm(shape, ip, ix, dt, rhs)
    bound = oracle_spmm(shape, ip, ix, np.abs(dt), np.abs(rhs))
    assert np.all(np.abs(got - ref) <= TOL * bound)
    m = DeviceCsMat.from_host(*as_csr(golden["mat3"]))           # 5 x 4
    with pytest.raises(SprsHipError, match="Dimension mismatch") as e:      # prod.rs:199-201
        prod.csr_mulacc_dense_rowmaj(m, prod.DeviceMat(5, 3), prod.DeviceMat(5, 3))
    assert e.value.status == _ffi.DIM_MISMATCH
    with pytest.raises(SprsHipError, match="Dimension mismatch"):
        prod.csr_mulacc_dense_rowmaj(m, prod.DeviceMat(4, 3), prod.DeviceMat(5, 2))
    shape, ip, ix, dt = as_csr(golden["mat1_csc"])
    csc = DeviceCsMat.from_host(shape, ip, ix, dt, storage=_ffi.CSC)
    with pytest.raises(SprsHipError, match="Storage mismatch"):             # prod.rs:202
        prod.csr_mulacc_dense_rowmaj(csc, prod.DeviceMat(5, 2), prod.DeviceMat(5, 2))
    # both wrong: the reference asserts the dimensions first and the storage last (prod.rs:199-202), and so does every mirror
    with pytest.raises(SprsHipError, match="Dimension mismatch"):
        prod.csr_mulacc_dense_rowmaj(csc, prod.DeviceMat(4, 2), prod.DeviceMat(5, 2))
    with pytest.raises(SprsHipError, match="Dimension mismatch"):
        prod.csc_mulacc_dense_colmaj(m, prod.DeviceMat(3, 2), prod.DeviceMat(5, 2))
    # a result that lies inside the right-hand side is refused (as for the vectors of the SpMV entries)
    sq = DeviceCsMat.eye(6)
    buf = prod.DeviceMat(6, 4)
    with pytest.raises(SprsHipError) as e:
        prod.csr_mulacc_dense_rowmaj(sq, buf, buf)
    assert e.value.status == _ffi.INVALID_ARG
    # ... but two element-disjoint views of ONE buffer are legal, as ndarray views are for the reference:
    # rhs = buf[:, 0:k], out = buf[:, k:2k] with pitch 2k (row-major), and the same as column blocks (column-major)
    import ctypes as C
    from sprs_amd.device import DeviceVec
    sq2 = DeviceCsMat.from_host((6, 6), np.arange(7, dtype=np.uint64), np.array([5, 4, 3, 2, 1, 0], dtype=np.uint64),
                                np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0]))          # a scaled row reversal
    for layout, ld in ((_ffi.ROW_MAJOR, 8), (_ffi.COL_MAJOR, 12)):
        host = rng.standard_normal(48)
        both = DeviceVec.from_host(host)
        off = 4 if layout == _ffi.ROW_MAJOR else 6                     # row-major: columns 4..7 of every 8-wide row; column-major: rows 6..11 of every 12-high column
        _ffi.check(_ffi.lib.sprs_hip_csmat_mulacc_dense_f64(sq2._h, C.c_void_p(both.ptr), 6, 4, layout, ld, C.c_void_p(both.ptr + off * 8), 6, layout, ld, 0, None))
        got = both.to_host()
        if layout == _ffi.ROW_MAJOR:
            v = got.reshape(6, 8)
            src, dst = host.reshape(6, 8)[:, :4], v[:, 4:]
            assert np.array_equal(v[:, :4], src)
        else:
            v = got.reshape(4, 12).T                                   # 12 x 4, column-major storage
            src, dst = host.reshape(4, 12).T[:6, :], v[6:, :]
            assert np.array_equal(v[:6, :], src)
        assert np.array_equal(dst, np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])[:, None] * src[::-1, :])
        # the same pitch with views that DO share elements is still refused
        with pytest.raises(SprsHipError) as e:
            _ffi.check(_ffi.lib.sprs_hip_csmat_mulacc_dense_f64(sq2._h, C.c_void_p(both.ptr), 6, 4, layout, ld, C.c_void_p(both.ptr + (off - 1) * 8), 6, layout, ld, 0, None))
        assert e.value.status == _ffi.INVALID_ARG


def test_hypersparse_operator_form(hip):
    """many more rows than entries: the operator form clears the result in one piece and runs the accumulate
    kernels on it — same values, every empty row +0.0 — for both result layouts (row-major from 8 columns, `.f()` below), a
    row-major and a column-major rhs, and rows at both ends of the matrix empty"""
    from sprs_amd import prod
    from sprs_amd.device import DeviceCsMat
    rng = np.random.default_rng(41)
    rows, cols, nnz = 300000, 5000, 700
    r = np.sort(rng.choice(np.arange(100, rows - 100), size=nnz // 2, replace=False))
    lens = np.zeros(rows, dtype=np.int64)
    lens[r] = rng.integers(1, 4, size=r.size)
    ip = np.zeros(rows + 1, dtype=np.uint64)
    ip[1:] = np.cumsum(lens)
    ix = np.concatenate([np.sort(rng.choice(cols, size=l, replace=False)) for l in lens[r]]).astype(np.uint64)
    dt = rng.standard_normal(ix.size)
    a = DeviceCsMat.from_host((rows, cols), ip, ix, dt)
    for k in (3, 16):
        rhs = rng.standard_normal((cols, k))
        ref = oracle_spmm((rows, cols), ip, ix, dt, rhs)
        for col_major in (False, True):
            out = (a * prod.DeviceMat.from_host(rhs, col_major=col_major)).to_host()
            assert rel_err(out, ref) <= TOL
            assert not out[lens == 0].any() and not np.signbit(out[lens == 0]).any()


def test_dense_dispatch_below_the_abi(hip):
    """`&CsMat * &Array2` / `&CsMat * &Array1` / `Array2::dot(&CsMat)` dispatched by the LIBRARY (csmat.rs:1989-2160):
    both storages, both rhs layouts, both result layouts (row-major from 8 columns, `.f()` below), the accumulate kernels of
    prod.rs with explicit layouts, the CSC -> CSR copy cached in the handle (second product of the same handle; refresh)."""
    import ctypes as C
    import scipy.sparse as sp
    from sprs_amd import _ffi, prod
    from sprs_amd.device import DeviceCsMat, DeviceVec, CSC
    rng = np.random.default_rng(12)
    u = lambda v: np.asarray(v, dtype=np.uint64)
    m = sp.random(700, 500, density=0.03, random_state=9, format="csr")
    m.data[:] = rng.standard_normal(m.nnz)
    m.sort_indices()
    mc = m.tocsc()
    mc.sort_indices()
    a_csr = DeviceCsMat.from_host((700, 500), u(m.indptr), u(m.indices), m.data)
    a_csc = DeviceCsMat.from_host((700, 500), u(mc.indptr), u(mc.indices), mc.data, storage=CSC)
    for a in (a_csr, a_csc):
        for k in (1, 3, 7, 8, 20):
            rhs = rng.standard_normal((500, k))
            ref = oracle_spmm((700, 500), u(m.indptr), u(m.indices), m.data, rhs)
            for rhs_col_major in (False, True):
                out = a * prod.DeviceMat.from_host(rhs, col_major=rhs_col_major)
                assert out.col_major == (k < 8)                       # csmat.rs:2002-2045: `.f()` below 8 columns
                assert rel_err(out.to_host(), ref) <= TOL
                for out_col_major in (False, True):                   # the accumulate kernels, every layout pair
                    out0 = rng.standard_normal((700, k))
                    acc = prod.DeviceMat.from_host(out0, col_major=out_col_major)
                    kernel = {(False, False): prod.csr_mulacc_dense_rowmaj, (False, True): prod.csr_mulacc_dense_colmaj,
                              (True, False): prod.csc_mulacc_dense_rowmaj, (True, True): prod.csc_mulacc_dense_colmaj}[(a.is_csc(), out_col_major)]
                    kernel(a, prod.DeviceMat.from_host(rhs, col_major=rhs_col_major), acc)
                    ref_acc = oracle_spmm((700, 500), u(m.indptr), u(m.indices), m.data, rhs, out0)
                    assert rel_err(acc.to_host(), ref_acc) <= TOL
        x = rng.standard_normal(500)
        y = (a * DeviceVec.from_host(x)).to_host()                    # `&A * &x`, CSC included (csmat.rs:2140-2156)
        assert rel_err(y, m @ x) <= TOL
    # prod::mul_acc_mat_vec_csc and its contract (prod.rs:88-92)
    y0 = rng.standard_normal(700)
    yv = DeviceVec.from_host(y0)
    prod.mul_acc_mat_vec_csc(a_csc, DeviceVec.from_host(x), yv)
    assert rel_err(yv.to_host(), y0 + m @ x) <= TOL
    with pytest.raises(hip.SprsHipError) as e:
        prod.mul_acc_mat_vec_csc(a_csr, DeviceVec.from_host(x), yv)
    assert e.value.status == _ffi.STORAGE_MISMATCH
    with pytest.raises(hip.SprsHipError) as e:
        prod.mul_acc_mat_vec_csc(a_csc, DeviceVec.from_host(np.zeros(499)), yv)
    assert e.value.status == _ffi.DIM_MISMATCH
    with pytest.raises(hip.SprsHipError) as e:                         # the twin of mul_acc_mat_vec_csr keeps ITS storage assert
        prod.mul_acc_mat_vec_csr(a_csc, DeviceVec.from_host(x), yv)
    assert e.value.status == _ffi.STORAGE_MISMATCH
    # dense . sparse (csmat.rs:2050-2117), both storages of the sparse operand, both layouts of the dense one
    for a, ms in ((a_csr, m), (a_csc, m)):
        for k in (3, 9):
            lhs = rng.standard_normal((k, 700))
            for cm in (False, True):
                got = prod.dense_dot_csmat(prod.DeviceMat.from_host(lhs, col_major=cm), a).to_host()
                assert got.shape == (k, 500) and rel_err(got, lhs @ ms.toarray()) <= 1e-9
    # a wrapped CSC handle whose values change in place: refresh drops the cached CSR copy
    import torch
    if not torch.cuda.is_available():                                  # (the CPU kernel emulator runs this test up to here)
        return
    dev = torch.device("cuda", 0)
    ip = torch.from_numpy(mc.indptr.astype(np.int64)).to(dev)
    ix = torch.from_numpy(mc.indices.astype(np.int64)).to(dev)
    dt = torch.from_numpy(mc.data.copy()).to(dev)
    w = DeviceCsMat.wrap_torch((700, 500), ip, ix, dt, storage=CSC)
    xv = DeviceVec.from_host(x)
    assert rel_err((w * xv).to_host(), m @ x) <= TOL
    dt.mul_(2.0)
    torch.cuda.synchronize()
    _ffi.check(_ffi.lib.sprs_hip_csmat_refresh(w._h))
    assert rel_err((w * xv).to_host(), 2.0 * (m @ x)) <= TOL


@pytest.mark.parametrize("stream_mode", [1, 0], ids=["stream", "chunks"])
def test_plan_built_on_a_nonblocking_stream(hip, stream_mode):
    """the SpMM plan made by a product on a torch stream (hipStreamNonBlocking: not ordered with the null stream) and used there
    at once is the plan of the null stream — the read-backs that size the chunk lists wait for that stream's kernels: same bits
    as a handle planned on the null stream"""
    import torch
    from sprs_amd import gen, prod
    from sprs_amd.device import DeviceCsMat
    n, k = 30000, 8
    indptr, indices, data = gen.rmat_csr(n, 10, seed=13)
    ip, ix, dt = indptr.numpy().astype(np.uint64), indices.numpy().astype(np.uint64), data.numpy()
    rhs = prod.DeviceMat.from_host(np.random.default_rng(5).random((n, k)) + 0.5)
    s = torch.cuda.Stream(device=torch.device("cuda", 0))
    out = []
    hip.set_option("spmm_stream", stream_mode)
    try:
        for stream in (s, None):
            a = DeviceCsMat.from_host((n, n), ip, ix, dt)
            res = prod.DeviceMat.from_host(np.zeros((n, k)))
            prod.csr_mulacc_dense_rowmaj(a, rhs, res, stream=stream)    # the plan is built and used on `stream`
            if stream is not None:
                stream.synchronize()
            out.append(res.to_host())
    finally:
        hip.set_option("spmm_stream", 1)
    assert np.array_equal(out[0], out[1])


# ---- exact-arithmetic seam cases ------------------------------------------------------------------------------------------
# Values, rhs and the initial result are nonzero integers in -4 .. 4: every product and every partial sum is an integer far below
# 2^53, so every order of the additions gives the same double and all four summation modes must equal the oracle BIT FOR BIT —
# one stray, stale or missing addend changes the result.  No tolerance anywhere below.
EXACT_MODES = (("stream", 0, 1, 2), ("stream-relaid-rhs", 0, 1, 1), ("chunks", 0, 0, 2), ("entry-order", 2048, 1, 2))
CHUNKS_ONLY, ENTRY_ORDER_ONLY = EXACT_MODES[2:3], EXACT_MODES[3:4]
K_CLASSES = [1, 7, 8, 9, 16, 17, 24, 32, 33, 64, 65, 129]       # every KP class, the 64-column block seam, 2nd / 3rd block of KP = 8
NAN_BITS = int(np.array([np.nan]).view(np.uint64)[0])
GUARD = 8                                                       # doubles before and after a caller's buffer


def exact_ints(rng, shape):
    return (rng.integers(1, 5, size=shape) * rng.choice([-1, 1], size=shape)).astype(np.float64)


def exact_csr(lens, cols, seed=0, idx=np.uint64, ptr=np.uint64, pins=()):
    """structure with the given row lengths: ascending distinct column ids (a start and a stride drawn per row); `pins` gives
    the ids of chosen rows, (row, ids)"""
    lens = np.asarray(lens, dtype=np.int64)
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


def int64_product(shape, ip, ix, dt, rhs, out0=None):
    """the product in int64 (prefix sums over the entries, differenced at the row bounds): no floating-point order at all"""
    p = ip.astype(np.int64)
    prod = dt.astype(np.int64)[:, None] * rhs.astype(np.int64)[ix.astype(np.int64)]
    cs = np.zeros((prod.shape[0] + 1, rhs.shape[1]), dtype=np.int64)
    np.cumsum(prod, axis=0, out=cs[1:])
    out = cs[p[1:]] - cs[p[:-1]]
    return out if out0 is None else out + out0.astype(np.int64)


def padded_image(rows, k, col_major, fill=None):
    """host image of a caller's buffer: GUARD doubles, a rows x k matrix with a padded pitch (k + 3 row-major, rows + 5
    column-major), GUARD doubles — every double NaN except the matrix cells when `fill` is given.  -> (flat, cells, pitch)"""
    ld = rows + 5 if col_major else k + 3
    lines = k if col_major else rows
    flat = np.full(2 * GUARD + lines * ld, np.nan)
    inside = np.zeros(flat.size, dtype=bool)
    for arr, val in ((inside, True), (flat, fill)):
        body = arr[GUARD:GUARD + lines * ld].reshape(lines, ld)
        cells = body[:, :rows].T if col_major else body[:, :k]
        if val is not None:
            cells[...] = val
    return flat, inside, ld


def cells_of(flat, rows, k, col_major):
    ld = rows + 5 if col_major else k + 3
    lines = k if col_major else rows
    body = flat[GUARD:GUARD + lines * ld].reshape(lines, ld)
    return body[:, :rows].T if col_major else body[:, :k]


def abi_product(a, shape, rhs, rhs_cm, out_cm, out0, accumulate, padded=True):
    """sprs_hip_csmat_mulacc_dense_f64 into a caller's buffer (NaN-filled for the operator form, `out0` in its cells for the
    accumulate form), rhs and result with padded pitches: -> the result cells, after checking that every gap cell and the guard
    doubles on both sides still hold their NaN bit pattern"""
    import ctypes as C
    from sprs_amd import _ffi
    from sprs_amd.device import DeviceVec
    rows, cols = shape
    k = rhs.shape[1]
    lay = lambda cm: _ffi.COL_MAJOR if cm else _ffi.ROW_MAJOR
    if padded:
        rflat, _, ld_r = padded_image(cols, k, rhs_cm, fill=rhs)
        oflat, inside, ld_o = padded_image(rows, k, out_cm, fill=out0 if accumulate else None)
        g = GUARD
    else:
        rflat = (np.asfortranarray(rhs).reshape(-1, order="F") if rhs_cm else rhs.reshape(-1)).copy()
        src = out0 if accumulate else np.full((rows, k), np.nan)
        oflat = (np.asfortranarray(src).reshape(-1, order="F") if out_cm else src.reshape(-1)).copy()
        ld_r, ld_o, g = (cols if rhs_cm else k), (rows if out_cm else k), 0
        if rflat.size == 0 or oflat.size == 0:
            return oflat.reshape(k, rows).T if out_cm else oflat.reshape(rows, k)
    rv, ov = DeviceVec.from_host(rflat), DeviceVec.from_host(oflat)
    _ffi.check(_ffi.lib.sprs_hip_csmat_mulacc_dense_f64(a._h, C.c_void_p(rv.ptr + 8 * g), cols, k, lay(rhs_cm), ld_r,
                                                        C.c_void_p(ov.ptr + 8 * g), rows, lay(out_cm), ld_o, accumulate, None))
    got = ov.to_host()
    assert np.array_equal(rv.to_host().view(np.uint64), rflat.view(np.uint64))      # the rhs is read only
    if not padded:
        return got.reshape(k, rows).T if out_cm else got.reshape(rows, k)
    outside = got.view(np.uint64)[~inside]
    bad = np.flatnonzero(outside != NAN_BITS)
    assert bad.size == 0, "%d gap / guard doubles of the caller's buffer were written, first at %s" % (bad.size, np.flatnonzero(~inside)[bad[:8]].tolist())
    return cells_of(got, rows, k, out_cm)


def check_spmm_exact(hip, shape, ip, ix, k, seed=0, modes=EXACT_MODES, tight_abi=False, what=""):
    """One structure through the summation modes of spmm.hip on ONE handle, every result equal to the oracle bit for bit: the
    operator and the accumulate form into tight row-major results, both forms through the ABI into NaN-filled caller buffers with
    padded pitches in both layouts (gaps and guards untouched), and a repeat with a fresh rhs (a cached plan, stale carries)."""
    from sprs_amd import prod
    from sprs_amd.device import DeviceCsMat
    fresh_blocks()
    rows, cols = shape
    rng = np.random.default_rng(seed)
    dt = exact_ints(rng, ix.size)
    rhs_a, rhs_b, out0 = exact_ints(rng, (cols, k)), exact_ints(rng, (cols, k)), exact_ints(rng, (rows, k))
    ip64, ix64 = ip.astype(np.uint64), ix.astype(np.uint64)
    lens = np.diff(ip.astype(np.int64))
    empty = lens == 0
    ref = {}
    for name, rhs in (("a", rhs_a), ("b", rhs_b)):              # before the device is touched: the oracle is the int64 product
        for acc, o0 in ((0, None), (1, out0)):
            r = oracle_spmm(shape, ip64, ix64, dt, rhs, o0)
            assert np.array_equal(r, int64_product(shape, ip, ix, dt, rhs, o0).astype(np.float64))
            assert not np.signbit(r[r == 0]).any()
            ref[name, acc] = r

    def same(got, want, how):
        bad = np.flatnonzero((got != want).any(axis=1) | np.isnan(got).any(axis=1))
        assert bad.size == 0 and np.array_equal(got, want), "%s %s, k = %d: %d rows differ, first rows %s of lengths %s: got %s, oracle %s" % (
            what, how, k, bad.size, bad[:4].tolist(), lens[bad[:4]].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist())

    a = DeviceCsMat.from_host(shape, ip, ix, dt)
    pairs = [(False, False), (True, True)] + ([(False, True)] if k < 8 else [])     # (below 8 columns two column-major operands run the SpMV)
    by_mode = {}
    try:
        for mode, long_row, stream, relayout in modes:
            hip.set_option("spmm_long_row", long_row)
            hip.set_option("spmm_stream", stream)
            hip.set_option("spmm_relayout", relayout)
            for name, rhs in (("a", rhs_a), ("b", rhs_b)):      # "b": the repeat on the same handle with a fresh rhs
                got = (a * prod.DeviceMat.from_host(rhs)).to_host()
                same(got, ref[name, 0], "%s, rhs %s, out = A rhs" % (mode, name))
                assert not np.signbit(got[empty]).any()         # empty rows: +0.0
                res = prod.DeviceMat.from_host(out0)
                prod.csr_mulacc_dense_rowmaj(a, prod.DeviceMat.from_host(rhs), res)
                got = res.to_host()
                same(got, ref[name, 1], "%s, rhs %s, out += A rhs" % (mode, name))
                assert np.array_equal(got[empty], out0[empty])  # empty rows untouched
                if name == "a":
                    by_mode[mode] = got
                    for rhs_cm, out_cm in pairs:
                        for padded in ((True, False) if tight_abi else (True,)):
                            for acc in (0, 1):
                                got = abi_product(a, shape, rhs, rhs_cm, out_cm, out0, acc, padded)
                                assert not np.isnan(got).any()
                                same(got, ref[name, acc], "%s, caller's buffer (rhs %s, out %s, %s, accumulate = %d)" % (
                                    mode, "col-major" if rhs_cm else "row-major", "col-major" if out_cm else "row-major",
                                    "padded" if padded else "tight", acc))
                                if not acc:
                                    assert not np.signbit(got[empty]).any()
    finally:
        hip.set_option("spmm_long_row", -1)
        hip.set_option("spmm_stream", 1)
        hip.set_option("spmm_relayout", 0)
    if "stream" in by_mode and "stream-relaid-rhs" in by_mode:  # from the rhs itself, from its re-laid-out copy: the same bits
        assert np.array_equal(by_mode["stream"], by_mode["stream-relaid-rhs"])
    return a


def pad_to(lens, offset, tile=256):
    """filler rows until the next row starts at `offset` of a tile"""
    need = (offset - sum(lens)) % tile
    if need > 40:
        lens += [need - 37, 37]
    elif need:
        lens.append(need)
    return lens


def kp_classes(k):
    """lane-group widths of the column blocks of a k-column product (blocks of 64; KP = the block's width rounded up to 8 .. 64)"""
    return {8 if kb <= 8 else 16 if kb <= 16 else 32 if kb <= 32 else 64 for kb in (min(64, k - j0) for j0 in range(0, k, 64))}


def tile_count_lens(nnz, seed, after):
    """rows of mostly 1 .. 3 entries, a few empty ones, and a row of 300 entries that crosses the last tile boundary: the last row,
    or (`after`) followed by up to 40 entries in short rows, as many as the last tile leaves room for, and three empty rows —
    row starts and empty rows that only the LAST tile meets, through tile_row[ntiles]"""
    last = (nnz - 1) // 256 * 256                                # first entry of the last tile
    m = min(40, nnz - 1 - last) if after else 0
    tail = []
    for l in [1, 2, 3, 1] * 5 + [3, 2]:
        l = min(l, m - sum(tail))
        if l:
            tail.append(l)
    rng = np.random.default_rng(seed)
    body = nnz - m - 300
    assert body < last <= nnz - m - 1                            # the row of 300 holds the entries on both sides of the boundary
    lens = rng.integers(1, 4, size=body)
    lens[rng.random(body) < 0.05] = 0
    cs = np.cumsum(lens)
    n = int(np.searchsorted(cs, body))
    lens = lens[:n + 1]
    lens[n] -= cs[n] - body
    lens = np.concatenate([lens, [300], tail, [0, 0, 0] if after else []]).astype(np.int64)
    assert lens.sum() == nnz
    return lens


BIG_COMBOS = [IDX_COMBOS[0], IDX_COMBOS[1]]


@pytest.mark.parametrize("idx,ptr", BIG_COMBOS)
@pytest.mark.parametrize("k", [8, 32])
@pytest.mark.parametrize("after", [False, True], ids=["row-last", "rows-after"])
@pytest.mark.parametrize("nnz", [65280, 65535, 65536, 65537])
def test_exact_tile_count_at_the_launch_seams(hip, nnz, after, k, idx, ptr):
    """ntiles = 255, 256, 256, 257: the last block of tile_rows_kernel (256 threads for ntiles + 1 values: tile_row[ntiles] has
    a block of its own when ntiles is a multiple of 256), a stream grid of whole and of partly filled workgroups, a block
    boundary of the fix-up grid.  (An unwritten tile_row[ntiles] shows only where the fresh block is not all-ones — any value
    >= rows acts as `rows` there; the emulator runs these cases a second time on zero-filled blocks for that.)"""
    lens = tile_count_lens(nnz, nnz, after)
    assert lens.sum() == nnz
    shape, ip, ix = exact_csr(lens, 5000, seed=nnz + k, idx=idx, ptr=ptr)
    check_spmm_exact(hip, shape, ip, ix, k, seed=k, what="nnz = %d" % nnz)


@pytest.mark.parametrize("idx,ptr", IDX_COMBOS)
@pytest.mark.parametrize("k", K_CLASSES)
def test_exact_tile_count_small(hip, k, idx, ptr):
    """nnz = 1, 255, 256, 257 in ONE row, alone and among empty rows: a single tile short of, at and one past its 256 entries"""
    for nnz in (1, 255, 256, 257):
        for lens in ([nnz], [0] * 5 + [nnz] + [0] * 7):
            shape, ip, ix = exact_csr(lens, 300, seed=nnz, idx=idx, ptr=ptr)
            check_spmm_exact(hip, shape, ip, ix, k, seed=nnz + k, what="nnz = %d in %d rows" % (nnz, len(lens)))


@pytest.mark.parametrize("idx,ptr", IDX_COMBOS)
@pytest.mark.parametrize("k", K_CLASSES)
def test_exact_fixup_span(hip, k, idx, ptr):
    """rows that cross tiles, at the fix-up's seams: a row that starts in a tile's last entry and goes on for exactly FIX_SPAN = 8
    tiles (one lane group adds its leads) and for 9 (the whole wave does, leads dealt to the G = 64 / KP groups); long rows that
    end on a tile's last entry and one entry later; long rows back to back, with and without an empty row between them; and
    lead counts of G - 1, G, G + 1, 3 G + 1 and the same around and beyond 8 for every KP class of this k"""
    edges = pad_to([], 255) + [1 + 8 * 256, 3]
    edges = pad_to(edges, 255) + [2 + 8 * 256]
    edges = pad_to(edges, 255) + [1 + 10 * 256, 2]               # ends on the last entry of a tile
    edges = pad_to(edges, 255) + [2 + 10 * 256]                  # ... and one entry past it
    edges = pad_to(edges, 100) + [2400, 2400, 0, 2400, 5]
    leads = []
    counts = set()
    for kp in kp_classes(k):
        g = 64 // kp
        counts |= {g - 1, g, g + 1, 3 * g + 1, 9, 8 + g, 9 + g, 9 + 3 * g + 1}
    for n in sorted(counts - {0}):
        leads = pad_to(leads, 255) + [1 + 256 * (n - 1) + 100]   # one entry, n - 1 whole tiles, 100 entries: n leads
    for what, lens in (("edges", edges), ("lead counts", leads)):
        shape, ip, ix = exact_csr(lens, 9500, seed=len(lens), idx=idx, ptr=ptr)
        check_spmm_exact(hip, shape, ip, ix, k, seed=k, what=what)


def row_start_cases():
    pw = [2, 4, 8, 16, 32, 64, 128]
    aligned = []
    for l in pw:                                                 # a row of l entries from a multiple of max(l, 32): a run boundary
        aligned = pad_to(aligned, 0, tile=max(l, 32)) + [l]
    shifted = [1]
    for l in pw:
        shifted = pad_to(shifted, 1, tile=max(l, 32)) + [l]
    return [
        ("300 one-entry rows", [1] * 300),                                          # a whole tile of row starts; runs of middle rows only
        ("one-entry rows between empty rows", [1, 0] * 200),
        ("70 empty rows first", [0] * 70 + [3, 1, 40, 2]),
        ("130 empty rows over a tile boundary", [200, 56] + [0] * 130 + [7, 300]),
        ("70 empty rows last", [5, 250, 1, 9] + [0] * 70),
        ("rows at run boundaries", aligned),
        ("rows one past run boundaries", shifted),
    ]


@pytest.mark.parametrize("idx,ptr", IDX_COMBOS)
@pytest.mark.parametrize("k", K_CLASSES)
def test_exact_many_row_starts_in_a_tile(hip, k, idx, ptr):
    """more than 64 row starts in a tile (the mark loop's second turn and further), runs made of middle rows only, runs of empty
    rows at the start, across a tile boundary and after the last entry, rows of 2 .. 128 entries at and one past run boundaries"""
    for i, (what, lens) in enumerate(row_start_cases()):
        shape, ip, ix = exact_csr(lens, 600, seed=i, idx=idx, ptr=ptr)
        check_spmm_exact(hip, shape, ip, ix, k, seed=10 * k + i, what=what)


@pytest.mark.parametrize("idx,ptr", IDX_COMBOS)
@pytest.mark.parametrize("k", K_CLASSES)
@pytest.mark.parametrize("cols", [4096, 4097, 8191, 12289])
def test_exact_relaid_rhs_beyond_one_block(hip, cols, k, idx, ptr):
    """the re-laid-out rhs with one, two and four blocks of 4096 rows: EVERY column is referenced (rows of 37 consecutive ids), one
    row holds 0, the powers of two, 4095, 4096 and cols - 1, one row crosses tiles; the copy and the rhs itself give the same bits"""
    special = sorted({0, 4095, min(4096, cols - 1), cols - 1} | {1 << b for b in range(14) if (1 << b) < cols})
    cover = [min(37, cols - c) for c in range(0, cols, 37)]
    lens = [len(special), 0] + cover + [600, 1]
    pins = [(0, special)] + [(2 + i, np.arange(37 * i, 37 * i + l)) for i, l in enumerate(cover)]
    shape, ip, ix = exact_csr(lens, cols, seed=cols, idx=idx, ptr=ptr, pins=pins)
    check_spmm_exact(hip, shape, ip, ix, k, seed=cols + k, what="cols = %d" % cols)


@pytest.mark.parametrize("idx,ptr", BIG_COMBOS)
@pytest.mark.parametrize("k", [3, 40])
def test_exact_chunk_grid_cap(hip, k, idx, ptr):
    """more chunks than the chunk kernel's grid has waves (65536): the grid-stride loop takes a second turn.  65600 rows of 1 or
    2 entries and rows of 513, 1024 and 1025 entries: the three chunks of the last of these are 65535, 65536, 65537, the row of
    1024 entries comes after them"""
    rng = np.random.default_rng(k)
    lens = rng.integers(1, 3, size=65600)
    lens[100], lens[65534], lens[65580] = 513, 1025, 1024
    first_chunk = np.concatenate([[0], np.cumsum((lens + 511) // 512)])
    assert first_chunk[65534] == 65535 and first_chunk[65580] > 65536 and first_chunk[-1] > 65536
    shape, ip, ix = exact_csr(lens, 3000, seed=k, idx=idx, ptr=ptr)
    check_spmm_exact(hip, shape, ip, ix, k, seed=k, modes=CHUNKS_ONLY, what="chunk grid cap")


@pytest.mark.parametrize("idx,ptr", BIG_COMBOS)
@pytest.mark.parametrize("k", [8, 16, 32, 64])
def test_exact_rows_grid_cap(hip, k, idx, ptr):
    """more rows than the entry-order kernel's grid has lane groups (2048 workgroups of 256 / KP: 65536 at KP = 8, 8192 at
    KP = 64), so every KP class takes its group-stride turn — the prefetched bounds, the second read of `out` in the accumulate
    form, rows of 2049 entries (left to the chunk kernels) met in a group's first and in later turns, an empty row after one"""
    rng = np.random.default_rng(k)
    lens = rng.integers(0, 4, size=65600)
    long_rows = [10, 5000, 8200, 16390, 32780, 65540]
    lens[long_rows] = 2049
    lens[[11, 65541]] = 0
    shape, ip, ix = exact_csr(lens, 3000, seed=k, idx=idx, ptr=ptr)
    check_spmm_exact(hip, shape, ip, ix, k, seed=k, modes=ENTRY_ORDER_ONLY, what="rows grid cap")


@pytest.mark.parametrize("idx,ptr", IDX_COMBOS)
@pytest.mark.parametrize("k", [3, 16, 70])
@pytest.mark.parametrize("extra", [4096, 4097], ids=["tiles-zero-the-empty-rows", "cleared-in-one-piece"])
def test_exact_hypersparse_threshold(hip, extra, k, idx, ptr):
    """nnz = 64 and rows = 4 nnz + 4096 | 4097: at and one past the threshold above which the operator form clears the result in
    one piece — all four ways of clearing it (tight / padded, row-major / column-major), gaps and guards of the padded ones kept"""
    nnz = 64
    rows = 4 * nnz + extra
    rng = np.random.default_rng(extra)
    lens = np.zeros(rows, dtype=np.int64)
    lens[np.sort(rng.choice(np.arange(50, rows - 50), size=32, replace=False))] = 2
    shape, ip, ix = exact_csr(lens, 500, seed=extra, idx=idx, ptr=ptr)
    assert ix.size == nnz
    check_spmm_exact(hip, shape, ip, ix, k, seed=k, tight_abi=True, what="rows = %d" % rows)


@pytest.mark.parametrize("idx,ptr", IDX_COMBOS)
@pytest.mark.parametrize("k", K_CLASSES)
def test_exact_nothing_stored(hip, k, idx, ptr):
    """nnz = 0: the operator form is +0.0 in every cell and nowhere else (tight and padded, both layouts), the accumulate form
    leaves every cell alone"""
    for rows in (1, 300):
        shape, ip, ix = exact_csr([0] * rows, 40, idx=idx, ptr=ptr)
        check_spmm_exact(hip, shape, ip, ix, k, seed=rows + k, tight_abi=True, what="no entries, %d rows" % rows)


@pytest.mark.parametrize("idx,ptr", IDX_COMBOS)
def test_exact_no_rows_or_no_columns_touch_nothing(hip, idx, ptr):
    """rows == 0 or k == 0: neither form writes a single double of the caller's buffer"""
    from sprs_amd.device import DeviceCsMat
    fresh_blocks()
    rng = np.random.default_rng(3)
    for lens, k in (([], 5), ([], 16), ([2, 0, 300, 1], 0), ([0, 0], 0)):
        shape, ip, ix = exact_csr(lens, 400, seed=1, idx=idx, ptr=ptr)
        a = DeviceCsMat.from_host(shape, ip, ix, exact_ints(rng, ix.size))
        rhs, out0 = exact_ints(rng, (400, k)), exact_ints(rng, (shape[0], k))
        for mode, long_row, stream, relayout in EXACT_MODES:
            hip.set_option("spmm_long_row", long_row)
            hip.set_option("spmm_stream", stream)
            hip.set_option("spmm_relayout", relayout)
            try:
                for rhs_cm, out_cm in ((False, False), (True, True), (False, True)):
                    for acc in (0, 1):
                        got = abi_product(a, shape, rhs, rhs_cm, out_cm, out0, acc)     # (checks gaps and guards)
                        assert got.shape == (shape[0], k)
            finally:
                hip.set_option("spmm_long_row", -1)
                hip.set_option("spmm_stream", 1)
                hip.set_option("spmm_relayout", 0)
