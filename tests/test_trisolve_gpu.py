"""GPU parity tests of the device sparse triangular solves (twins of lsolve_csr / usolve_csr / lsolve_csc / usolve_csc
_dense_rhs, sprs/src/sparse/linalg/trisolve.rs) against the plain-Python restatement of tests/trisolve_ref.py: every solution
bit for bit (np.array_equal on finite inputs), the level counts, the reference's Err(SingularMatrix) and asserts as errors.
(tests/test_trisolve_emu_cpu.py runs this file through the CPU emulator of the kernels as well.)"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import trisolve_ref as ref
from test_gauss_seidel_gpu import _random_system

pytestmark = pytest.mark.gpu

EMU = "emu" in os.path.basename(os.environ.get("SPRS_HIP_LIBRARY", ""))
KINDS = ["lsolve_csr", "usolve_csr", "lsolve_csc", "usolve_csc"]
WIDTHS = [(np.uint64, np.uint64), (np.uint32, np.uint64), (np.uint32, np.uint32)]


@pytest.fixture(scope="module")
def hip():
    import sprs_amd
    if sprs_amd.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X (no CPU fallback exists)")
    return sprs_amd


def arrays(a, kind):
    """the CSR or CSC arrays (sorted indices) of a scipy matrix, as the solve `kind` takes them"""
    m = a.tocsc() if kind.endswith("csc") else a.tocsr()
    m.sort_indices()
    return m.indptr.astype(np.uint64), m.indices.astype(np.uint64), m.data.astype(np.float64)


def device_mat(kind, n, ip, ix, dt, idx=np.uint64, ptr=np.uint64, validate=True):
    from sprs_amd.device import DeviceCsMat, CSC, CSR
    return DeviceCsMat.from_host((n, n), ip.astype(ptr), ix.astype(idx), dt, storage=CSC if kind.endswith("csc") else CSR,
                                 validate=validate)


def gpu_fn(kind):
    from sprs_amd import linalg
    return getattr(linalg, kind + "_dense_rhs")


def gpu_solve(kind, n, ip, ix, dt, b, idx=np.uint64, ptr=np.uint64):
    from sprs_amd.device import DeviceVec
    a = device_mat(kind, n, ip, ix, dt, idx, ptr)
    x = DeviceVec.from_host(b)
    res = gpu_fn(kind)(a, x)
    return x.to_host(), res


def check_against_restatement(kind, a, b, idx=np.uint64, ptr=np.uint64):
    n = a.shape[0]
    ip, ix, dt = arrays(a, kind)
    x_ref = ref.SOLVES[kind](n, ip, ix, dt, b)
    assert np.isfinite(x_ref).all()
    x, res = gpu_solve(kind, n, ip, ix, dt, b, idx, ptr)
    assert np.array_equal(x, x_ref)
    assert res.levels == ref.levels(kind, n, ip, ix)
    return x


def test_golden_systems(hip):
    """the reference's own unit tests, trisolve.rs:368-442"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trisolve_fixtures.json")
    systems = json.load(open(path))["systems"]
    assert sorted(s["solve"] for s in systems) == sorted(KINDS)
    for s in systems:
        ip, ix = np.array(s["indptr"], dtype=np.uint64), np.array(s["indices"], dtype=np.uint64)
        x, _ = gpu_solve(s["solve"], s["shape"][0], ip, ix, np.array(s["data"], dtype=np.float64), np.array(s["b"], dtype=np.float64))
        assert np.array_equal(x, np.array(s["x"], dtype=np.float64)), s["solve"]


def _cases():
    out = []
    for kind in KINDS:
        for n in (1, 63, 64, 65, 500):
            for idx, ptr in (WIDTHS if n == 65 else WIDTHS[:1]):
                out.append(pytest.param(kind, n, idx, ptr, id="%s-%d-%s-%s" % (kind, n, np.dtype(idx).name, np.dtype(ptr).name)))
    return out


@pytest.mark.parametrize("kind,n,idx,ptr", _cases())
def test_random_systems(hip, kind, n, idx, ptr):
    """full non-symmetric matrices: the other triangle is there and must be ignored; at n = 500 row n // 2 has more than one
    batch of eight on both sides of the diagonal"""
    a = _random_system(n, 11 + n, 0 if n == 1 else 4, 100 if n == 500 else 0)
    if n == 500:
        row = a.indices[a.indptr[n // 2]:a.indptr[n // 2 + 1]]
        assert (row < n // 2).sum() > 8 and (row > n // 2).sum() > 8
    check_against_restatement(kind, a, np.random.default_rng(n).standard_normal(n), idx, ptr)


@pytest.mark.parametrize("kind", ["lsolve_csr", "usolve_csr"])
def test_bidiagonal_chain(hip, kind):
    """every unknown waits for its neighbour: n levels, the dependencies run inside a wave and across waves"""
    import scipy.sparse as sp
    n = 130 if EMU else 200
    a = (sp.diags(np.full(n, 2.0)) + sp.diags(np.full(n - 1, -1.0), -1 if kind[0] == "l" else 1)).tocsr()
    ip, ix, dt = arrays(a, kind)
    b = np.arange(1, n + 1, dtype=np.float64)
    x, res = gpu_solve(kind, n, ip, ix, dt, b)
    assert res.levels == n
    assert np.array_equal(x, ref.SOLVES[kind](n, ip, ix, dt, b))


@pytest.mark.parametrize("kind", KINDS)
def test_dense_triangle(hip, kind):
    """rows of up to 130 entries (17 batches of eight), every unknown its own level"""
    import scipy.sparse as sp
    n = 130
    rng = np.random.default_rng(130)
    d = rng.uniform(-1.0, 1.0, (n, n))
    d = np.tril(d) if kind[0] == "l" else np.triu(d)
    d[np.arange(n), np.arange(n)] = np.abs(d).sum(axis=1) + 1.0
    x = check_against_restatement(kind, sp.csr_matrix(d), rng.standard_normal(n))
    ip, ix, _ = arrays(sp.csr_matrix(d), kind)
    assert ref.levels(kind, n, ip, ix) == n and np.isfinite(x).all()


@pytest.mark.parametrize("kind", KINDS)
def test_heat_system_triangles(hip, kind):
    """the lower and the upper part of the heat example's matrix: levels as the recurrence counts them"""
    from oracle import oracle
    import scipy.sparse as sp
    r = 24 if EMU else 96
    shape, ip, ix, dt = oracle.grid_laplacian(r, r)
    a = sp.csr_matrix((dt, ix.astype(np.int64), ip.astype(np.int64)), shape=shape)
    part = sp.tril(a) if kind[0] == "l" else sp.triu(a)
    check_against_restatement(kind, part.tocsr(), np.random.default_rng(r).standard_normal(r * r))


def test_walk_direction(hip):
    """usolve_csr adds row r's products by ascending column, usolve_csc by descending column (its columns run n-1 .. 0):
    one matrix, two different bit patterns, and the device reproduces each"""
    n = 70
    a = _random_system(n, 3, 4)
    b = np.random.default_rng(n).standard_normal(n)
    refs = {}
    for kind in ("usolve_csr", "usolve_csc"):
        ip, ix, dt = arrays(a, kind)
        refs[kind] = ref.SOLVES[kind](n, ip, ix, dt, b)
    assert not np.array_equal(refs["usolve_csr"], refs["usolve_csc"])
    assert np.allclose(refs["usolve_csr"], refs["usolve_csc"], rtol=0, atol=1e-12)
    for kind in ("usolve_csr", "usolve_csc"):
        assert np.array_equal(check_against_restatement(kind, a, b), refs[kind])


def test_transposed_factor(hip):
    """L^T x = b without a copy: the transpose view of a CSR lower factor is a CSC handle of an upper triangular matrix"""
    import scipy.sparse as sp
    from sprs_amd.device import DeviceVec
    n = 90
    low = sp.tril(_random_system(n, 5, 4)).tocsr()
    low.sort_indices()
    ip, ix, dt = low.indptr.astype(np.uint64), low.indices.astype(np.uint64), low.data
    b = np.random.default_rng(n).standard_normal(n)
    # the CSR arrays of L are the CSC arrays of L^T
    x_ref = ref.usolve_csc_dense_rhs(n, ip, ix, dt, b)
    handle = device_mat("lsolve_csr", n, ip, ix, dt)
    view = handle.transpose_view()
    assert view.is_csc()
    x = DeviceVec.from_host(b)
    res = gpu_fn("usolve_csc")(view, x)
    assert np.array_equal(x.to_host(), x_ref)
    assert res.levels == ref.levels("usolve_csc", n, ip, ix)
    assert np.abs(low.T @ x_ref - b).max() < 1e-12


class _Wrapped:
    """three raw device buffers behind sprs_hip_csmat_wrap_device: a handle whose values the test can change in place"""

    def __init__(self, kind, n, ip, ix, dt):
        from sprs_amd import _ffi
        from sprs_amd.device import DeviceCsMat, CSC, CSR
        self.lib, self.bufs = _ffi.lib, []
        ptrs = [self._upload(arr) for arr in (ip, ix, dt)]
        h = C.c_void_p()
        _ffi.check(self.lib.sprs_hip_csmat_wrap_device(C.byref(h), CSC if kind.endswith("csc") else CSR, n, n, ix.size, ptrs[0], 8,
                                                       ptrs[1], 8, ptrs[2]))
        self.mat = DeviceCsMat(h.value, keep=self)
        self.data = ptrs[2]

    def _upload(self, arr):
        from sprs_amd import _ffi
        arr = np.ascontiguousarray(arr)
        p = C.c_void_p()
        _ffi.check(self.lib.sprs_hip_malloc(C.byref(p), max(arr.nbytes, 8)))
        self.bufs.append(p)
        _ffi.check(self.lib.sprs_hip_memcpy_h2d(p, C.c_void_p(arr.ctypes.data), arr.nbytes))
        return p

    def set_values(self, dt):
        from sprs_amd import _ffi
        dt = np.ascontiguousarray(dt, dtype=np.float64)
        _ffi.check(self.lib.sprs_hip_memcpy_h2d(self.data, C.c_void_p(dt.ctypes.data), dt.nbytes))
        self.mat.refresh()

    def free(self):
        self.mat = None
        for p in self.bufs:
            self.lib.sprs_hip_free(p)
        self.bufs = []


@pytest.mark.parametrize("kind", ["usolve_csr", "lsolve_csc"])
def test_reuse_and_refresh(hip, kind):
    """two solves on one handle give the same bits; values changed in place + refresh give the new matrix's solution (for the
    CSC handle the cached CSR form has to go, not only the row order)"""
    from sprs_amd.device import DeviceVec
    n = 100
    a = _random_system(n, 8, 4)
    ip, ix, dt = arrays(a, kind)
    b = np.random.default_rng(1).standard_normal(n)
    w = _Wrapped(kind, n, ip, ix, dt)
    try:
        outs = []
        for _ in range(2):
            x = DeviceVec.from_host(b)
            gpu_fn(kind)(w.mat, x)
            outs.append(x.to_host())
        assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], ref.SOLVES[kind](n, ip, ix, dt, b))
        dt2 = dt * np.random.default_rng(2).uniform(1.0, 1.01, dt.size)      # still strictly diagonally dominant
        x_new = ref.SOLVES[kind](n, ip, ix, dt2, b)
        assert not np.array_equal(x_new, outs[0])
        w.set_values(dt2)
        x = DeviceVec.from_host(b)
        gpu_fn(kind)(w.mat, x)
        assert np.array_equal(x.to_host(), x_new)
    finally:
        w.free()


@pytest.mark.parametrize("solve_first", [True, False])
def test_lower_plan_is_shared_with_gauss_seidel(hip, solve_first):
    """lsolve_csr runs on the Gauss-Seidel level order: either call may build it, both stay bit-identical to the CPU"""
    from oracle import oracle
    from sprs_amd.device import DeviceVec
    from sprs_amd.linalg import gauss_seidel
    n = 150
    a = _random_system(n, 21, 4)
    ip, ix, dt = arrays(a, "lsolve_csr")
    rng = np.random.default_rng(4)
    b, x0 = rng.standard_normal(n), rng.standard_normal(n)
    handle = device_mat("lsolve_csr", n, ip, ix, dt)
    x_gs_ref, _ = oracle.gauss_seidel((n, n), ip, ix, dt, x0, b, 3, -1.0)
    x_tri_ref = ref.lsolve_csr_dense_rhs(n, ip, ix, dt, b)

    def solve():
        x = DeviceVec.from_host(b)
        res = gpu_fn("lsolve_csr")(handle, x)
        assert np.array_equal(x.to_host(), x_tri_ref)
        return res.levels

    def sweep():
        x = DeviceVec.from_host(x0)
        res = gauss_seidel(handle, x, DeviceVec.from_host(b), 3, -1.0)
        assert np.array_equal(x.to_host(), x_gs_ref)
        return res.levels

    got = [solve(), sweep()] if solve_first else [sweep(), solve()]
    assert got[0] == got[1] == ref.levels("lsolve_csr", n, ip, ix)


def test_contract_violations(hip):
    """check_solver_dimensions (trisolve.rs:10-21), the storage asserts (trisolve.rs:42, 98, 174, 232), uplo at the C level"""
    from sprs_amd import _ffi
    from sprs_amd.device import DeviceCsMat, DeviceVec
    rect = DeviceCsMat.from_host((2, 3), np.array([0, 1, 2], dtype=np.uint64), np.array([0, 1], dtype=np.uint64), np.ones(2))
    with pytest.raises(_ffi.SprsHipError) as e:
        gpu_fn("lsolve_csr")(rect, DeviceVec.zeros(2))
    assert e.value.status == _ffi.DIM_MISMATCH and "Non square matrix passed to solver" in str(e.value)
    eye = DeviceCsMat.eye(4)
    with pytest.raises(_ffi.SprsHipError) as e:
        gpu_fn("usolve_csr")(eye, DeviceVec.zeros(5))
    assert e.value.status == _ffi.DIM_MISMATCH and "Dimension mismatch" in str(e.value)
    x = DeviceVec.zeros(4)
    assert _ffi.lib.sprs_hip_trisolve_f64(eye._h, 7, C.c_void_p(x.ptr), 4, None, None) == _ffi.INVALID_ARG
    assert _ffi.lib.sprs_hip_trisolve_f64(eye._h, _ffi.LOWER, None, 4, None, None) == _ffi.INVALID_ARG
    for kind in ("lsolve_csc", "usolve_csc"):
        with pytest.raises(_ffi.SprsHipError) as e:
            gpu_fn(kind)(eye, x)
        assert e.value.status == _ffi.STORAGE_MISMATCH and "Storage mismatch" in str(e.value)
    csc = eye.to_other_storage()
    for kind in ("lsolve_csr", "usolve_csr"):
        with pytest.raises(_ffi.SprsHipError) as e:
            gpu_fn(kind)(csc, x)
        assert e.value.status == _ffi.STORAGE_MISMATCH
    # n == 0: nothing to do
    empty = DeviceCsMat.from_host((0, 0), np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint64), np.zeros(0))
    assert gpu_fn("lsolve_csr")(empty, DeviceVec(0)).levels == 0


def _singular_system(n, missing, zeros):
    """a random system whose diagonal entries `missing` are not stored and whose diagonal entries `zeros` are stored 0.0"""
    import scipy.sparse as sp
    a = _random_system(n, 31, 3).tocoo()
    keep = ~((a.row == a.col) & np.isin(a.row, missing))
    data = np.where((a.row == a.col) & np.isin(a.row, zeros), 0.0, a.data)
    r, c, d = a.row[keep], a.col[keep], data[keep]
    order = np.lexsort((c, r))
    ip = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.uint64)
    csr = (ip, c[order].astype(np.uint64), d[order])
    order = np.lexsort((r, c))
    ip = np.concatenate([[0], np.cumsum(np.bincount(c, minlength=n))]).astype(np.uint64)
    csc = (ip, r[order].astype(np.uint64), d[order])
    return csr, csc


@pytest.mark.parametrize("kind", KINDS)
def test_singular_matrices(hip, kind):
    """a diagonal that is not stored, an explicit 0.0 (and -0.0), and two singular indices at once: the index and the reason
    of the reference (the first in ITS processing order: the smallest for lsolve, the largest for usolve)"""
    from sprs_amd import _ffi
    from sprs_amd.device import DeviceVec
    n = 80
    b = np.random.default_rng(9).standard_normal(n)
    for missing, zeros, minus in (([37], [], False), ([], [41], False), ([], [41], True), ([12], [70], False), ([70], [12], False),
                                  ([0], [], False), ([], [n - 1], False)):
        csr, csc = _singular_system(n, missing, zeros)
        ip, ix, dt = csc if kind.endswith("csc") else csr
        if minus:
            dt = np.where(dt == 0.0, -0.0, dt)
        with pytest.raises(ref.Singular) as want:
            ref.SOLVES[kind](n, ip, ix, dt, b)
        assert want.value.index == (max if kind[0] == "u" else min)(missing + zeros)
        a = device_mat(kind, n, ip, ix, dt)
        with pytest.raises(_ffi.SprsHipError) as e:
            gpu_fn(kind)(a, DeviceVec.from_host(b))
        assert e.value.status == _ffi.SINGULAR_MATRIX
        assert e.value.index == want.value.index
        assert str(want.value) in str(e.value)                       # "Singular matrix at index {} ({reason})", errors.rs:87-92
        structural = kind.endswith("csc") and want.value.index in missing
        assert e.value.reason == ("structural" if structural else "numeric")
        assert ("structural" in want.value.reason) == structural


def test_nan_diagonal_is_not_singular(hip):
    """`diag == 0` is false for a NaN (trisolve.rs:64): the solve returns Ok with NaNs where the reference has them"""
    n = 40
    csr, _ = _singular_system(n, [], [20])
    ip, ix, dt = csr
    dt = np.where(dt == 0.0, np.nan, dt)
    b = np.ones(n)
    x_ref = ref.lsolve_csr_dense_rhs(n, ip, ix, dt, b)
    x, _ = gpu_solve("lsolve_csr", n, ip, ix, dt, b)
    assert np.isnan(x_ref[20]) and np.array_equal(np.isnan(x), np.isnan(x_ref))
    ok = ~np.isnan(x_ref)
    assert np.array_equal(x[ok], x_ref[ok])


@pytest.mark.parametrize("kind", ["lsolve_csr", "usolve_csc"])
def test_singular_head_of_a_chain(hip, kind):
    """the first unknown of a 200-row chain is singular: it publishes a NaN, its dependents finish, the call returns the error"""
    import scipy.sparse as sp
    from sprs_amd import _ffi
    from sprs_amd.device import DeviceVec
    n = 200
    lower = kind[0] == "l"
    d = np.full(n, 2.0)
    head = 0 if lower else n - 1
    d[head] = 0.0
    a = sp.coo_matrix((np.concatenate([d, np.full(n - 1, -1.0)]),
                       (np.concatenate([np.arange(n), np.arange(1, n) if lower else np.arange(n - 1)]),
                        np.concatenate([np.arange(n), np.arange(n - 1) if lower else np.arange(1, n)]))), shape=(n, n))
    m = a.tocsc() if kind.endswith("csc") else a.tocsr()              # (tocsr / tocsc keep the explicit zero)
    m.sort_indices()
    ip, ix, dt = m.indptr.astype(np.uint64), m.indices.astype(np.uint64), m.data
    assert ix.size == 2 * n - 1
    handle = device_mat(kind, n, ip, ix, dt)
    with pytest.raises(_ffi.SprsHipError) as e:
        gpu_fn(kind)(handle, DeviceVec.from_host(np.ones(n)))
    assert e.value.status == _ffi.SINGULAR_MATRIX and e.value.index == head and e.value.reason == "numeric"
