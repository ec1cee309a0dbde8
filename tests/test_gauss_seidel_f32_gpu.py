"""GPU parity tests of the f32 Gauss-Seidel (sprs_hip_gauss_seidel_f32 behind sprs_amd.linalg.gauss_seidel on a DeviceCsMatF32)
against the np.float32 restatement of heat.rs:103-139 in tests/f32_solve_ref.py: every iterate bit for bit, the sweep counts,
the reference's panics as errors.  The systems are those of tests/test_gauss_seidel_gpu.py cast to f32.

The convergence scalar e = sqrt(sum_i ((A x)_i - rhs_i)) is compared through a DERIVED bound, not a measured one: the device sums
in a fixed tree and the reference in ndarray's order, and long rows of the f32 SpMV are not the reference's chain.  Both are sums of
the same n + nnz terms in some order with at most n + m + 2 roundings on any path to the result (m = the longest row: its chain;
one subtraction; the sum over n rows; the square root squared back), so with u = 2^-24 and
S = sum_i (sum_k |a_ik| |x_k| + |rhs_i|) in f64:   |e_gpu^2 - e_ref^2| <= 2 (n + m + 2) u S.
Where the reference's sum is below -bound both scalars are NaN; a sum within the bound of zero decides nothing, and the tests
that pin the scalar assert on the CPU that their inputs stay clear of it.
(tests/test_solve_f32_emu_cpu.py runs this file through the CPU emulator of the kernels as well.)"""
import numpy as np
import pytest

import f32_solve_ref as ref
from test_gauss_seidel_gpu import EMU, _random_system, heat_system

pytestmark = pytest.mark.gpu

F = np.float32
U = 2.0 ** -24


@pytest.fixture(scope="module")
def hip():
    import sprs_amd
    if sprs_amd.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X (no CPU fallback exists)")
    if not hasattr(sprs_amd._ffi.lib, "sprs_hip_gauss_seidel_f32"):
        pytest.fail("the library has no sprs_hip_gauss_seidel_f32")
    return sprs_amd


def heat32(rows, idx=np.uint64, ptr=np.uint64):
    shape, ip, ix, dt, rhs = heat_system(rows, idx, ptr)
    return shape, ip, ix, dt.astype(np.float32), rhs.astype(np.float32)


def gpu_gs(shape, ip, ix, dt, x0, rhs, max_iter, eps):
    from sprs_amd.device import DeviceCsMatF32, DeviceVecF32
    from sprs_amd.linalg import gauss_seidel
    assert dt.dtype == x0.dtype == rhs.dtype == np.float32
    a = DeviceCsMatF32.from_host(shape, ip, ix, dt)
    x = DeviceVecF32.from_host(x0)
    res = gauss_seidel(a, x, DeviceVecF32.from_host(rhs), max_iter, eps)
    out = x.to_host()
    assert out.dtype == np.float32
    return out, res


def error_bound(ip, ix, dt, x, rhs):
    """2 (n + m + 2) u S for the iterate x (module docstring), in f64"""
    ip64 = np.asarray(ip).astype(np.int64)
    n = ip64.size - 1
    m = int(np.diff(ip64).max()) if n else 0
    absx = np.abs(x.astype(np.float64))
    terms = np.abs(dt.astype(np.float64)) * absx[np.asarray(ix).astype(np.int64)]
    S = terms.sum() + np.abs(rhs.astype(np.float64)).sum()
    return 2.0 * (n + m + 2) * U * S


def check_error(e_gpu, sum_ref, bound, must_decide):
    """the device's scalar against the restatement's residual SUM (f32) under the derived bound"""
    sum_ref = float(sum_ref)
    print("error scalar: e_gpu^2 = %r, sum_ref = %r, bound = %r" % (float(e_gpu) ** 2, sum_ref, bound))
    if must_decide:
        assert abs(sum_ref) > bound, "the inputs leave the sign of the residual sum undecided"
    if sum_ref < -bound:
        assert np.isnan(e_gpu)
    elif sum_ref > bound:
        assert abs(float(e_gpu) ** 2 - float(F(np.sqrt(F(sum_ref)))) ** 2) <= bound
    else:
        assert np.isnan(e_gpu) or float(e_gpu) ** 2 <= 2.0 * bound


def test_heat_example(hip):
    """the example itself (heat.rs:141-157) in f32: 10 x 10 grid, up to 300 sweeps.  eps is chosen on the CPU: the smallest of a
    few candidates for which every sweep up to the converging one is DECIDED under the bound — its sum clearly above eps^2,
    clearly negative (NaN), or clearly below eps^2 — so the device must stop in the same sweep.  (The bound is about 0.07 here:
    the example's own eps = 1e-8 lies far below what f32 can decide.)"""
    shape, ip, ix, dt, rhs = heat32(10)
    bounds = {}
    trace = ref.gauss_seidel(shape, ip, ix, dt, np.zeros(100, dtype=np.float32), rhs, 300, -1.0,
                             on_sweep=lambda k, x: bounds.__setitem__(k, error_bound(ip, ix, dt, x, rhs)))
    assert not trace.converged and len(trace.sums) == 301

    def decided(eps):
        """the sweep (0-based) after which error < eps, when every scalar up to it is decided; else None"""
        e2 = float(F(eps)) ** 2
        for k in range(1, 301):
            s, b = float(trace.sums[k]), bounds[k]
            if s > e2 + b or s < -b:
                continue                                     # not converged on both sides (NaN < eps is false)
            if b < s and s + b < e2:
                return k - 1
            return None
        return None

    eps = next((e for e in (0.5, 0.7, 1.0, 1.5, 2.0, 3.0) if decided(e) is not None and decided(e) >= 3), None)
    assert eps is not None, "no eps keeps the restatement's error sequence clear of the bound"
    want = ref.gauss_seidel(shape, ip, ix, dt, np.zeros(100, dtype=np.float32), rhs, 300, eps)
    assert want.converged and want.iterations == decided(eps)
    x, res = gpu_gs(shape, ip, ix, dt, np.zeros(100, dtype=np.float32), rhs, 300, eps)
    assert res.converged and res.iterations == want.iterations
    assert np.array_equal(x, want.x)
    check_error(res.error, want.sums[-1], error_bound(ip, ix, dt, want.x, rhs), True)
    assert res.error == float(F(res.error))                    # the f32 value widened
    assert res.levels == 16


_ITERATES = {}


@pytest.mark.parametrize("sweeps", [1, 2, 7])
def test_every_iterate_bit_for_bit(hip, sweeps):
    """a grid with more rows than one wave chunk and more levels than waves in a workgroup; Err(error) after k sweeps"""
    rows = 24 if EMU else 96
    shape, ip, ix, dt, rhs = heat32(rows)
    x0 = np.random.default_rng(3).standard_normal(rows * rows).astype(np.float32)
    if not _ITERATES:                                          # one run of the restatement serves the three cases
        ref.gauss_seidel(shape, ip, ix, dt, x0, rhs, 7, -1.0, on_sweep=lambda k, x: _ITERATES.__setitem__(k, x))
    x, res = gpu_gs(shape, ip, ix, dt, x0, rhs, sweeps, -1.0)
    assert not res.converged and res.iterations == sweeps
    assert np.array_equal(x, _ITERATES[sweeps])
    s = ref.residual_sum(shape, ip, ix, dt, _ITERATES[sweeps], rhs)
    check_error(res.error, s, error_bound(ip, ix, dt, _ITERATES[sweeps], rhs), False)
    assert res.levels == 2 * rows - 4


@pytest.mark.parametrize("n,density,long_row", [(1, 0, 0), (63, 3, 0), (64, 2, 20), (500, 4, 100)])
def test_random_nonsymmetric_systems(hip, n, density, long_row):
    """rows whose columns before the diagonal are NOT mirrored by entries after it, rows of many entries, a single row"""
    a = _random_system(n, 11 + n, density, long_row)
    ip, ix, dt = a.indptr.astype(np.uint64), a.indices.astype(np.uint64), a.data.astype(np.float32)
    rng = np.random.default_rng(n)
    rhs, x0 = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    for sweeps in (1, 3):
        want = ref.gauss_seidel((n, n), ip, ix, dt, x0, rhs, sweeps, -1.0)
        x, res = gpu_gs((n, n), ip, ix, dt, x0, rhs, sweeps, -1.0)
        assert np.array_equal(x, want.x)
        assert not res.converged and res.iterations == sweeps
        check_error(res.error, want.sums[-1], error_bound(ip, ix, dt, want.x, rhs), False)


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_error_scalar(hip, sign):
    """the scalar itself, on inputs whose residual sum is far from zero on either side (asserted on the CPU): the 500-row system
    with its long row, a random vector x and rhs = A x -/+ 3 on every row, so sum(A x - rhs) is about +/- 1500.  Zero sweeps
    return the scalar of x as it stands (heat.rs:111, 138): finite for the positive sum, NaN for the negative one"""
    n = 500
    a = _random_system(n, 11 + n, 4, 100)
    ip, ix, dt = a.indptr.astype(np.uint64), a.indices.astype(np.uint64), a.data.astype(np.float32)
    assert int(np.diff(a.indptr).max()) > 64                   # (the 100 extra entries of row n // 2, duplicates merged)
    x0 = np.random.default_rng(n).standard_normal(n).astype(np.float32)
    rhs = (a.astype(np.float32).astype(np.float64) @ x0.astype(np.float64) - 3.0 * sign).astype(np.float32)
    want = ref.gauss_seidel((n, n), ip, ix, dt, x0, rhs, 0, 1e-3)
    x, res = gpu_gs((n, n), ip, ix, dt, x0, rhs, 0, 1e-3)
    assert np.array_equal(x, x0)
    assert (res.converged, res.iterations) == (want.converged, want.iterations) == (False, 0)
    assert (float(want.sums[-1]) > 0) == (sign > 0) and np.isnan(want.error) == (sign < 0)
    check_error(res.error, want.sums[-1], error_bound(ip, ix, dt, x0, rhs), True)


def test_lower_triangular_chain(hip):
    """bidiagonal matrix: every row waits for the one before it (n levels), adjacent 4-byte words inside and across waves"""
    import scipy.sparse as sp
    n = 200 if EMU else 1000
    a = (sp.diags(np.full(n, 2.0)) + sp.diags(np.full(n - 1, -1.0), -1)).tocsr()
    ip, ix, dt = a.indptr.astype(np.uint64), a.indices.astype(np.uint32), a.data.astype(np.float32)
    rhs = np.arange(1, n + 1, dtype=np.float32)
    want = ref.gauss_seidel((n, n), ip, ix, dt, np.zeros(n, dtype=np.float32), rhs, 2, -1.0)
    x, res = gpu_gs((n, n), ip, ix, dt, np.zeros(n, dtype=np.float32), rhs, 2, -1.0)
    assert res.levels == n
    assert np.array_equal(x, want.x)
    assert (res.converged, res.iterations) == (False, 2)


def test_zero_sweeps_returns_the_initial_error(hip):
    """max_iter = 0: Err(error of the start vector) (heat.rs:111, 138), x untouched"""
    shape, ip, ix, dt, rhs = heat32(8)
    x0 = np.linspace(20, 50, 64).astype(np.float32)           # the border rows alone make sum(A x0 - rhs) clearly positive
    want = ref.gauss_seidel(shape, ip, ix, dt, x0, rhs, 0, 1e-8)
    x, res = gpu_gs(shape, ip, ix, dt, x0, rhs, 0, 1e-8)
    assert np.array_equal(x, x0) and np.array_equal(want.x, x0)
    assert not res.converged and res.iterations == 0
    check_error(res.error, want.sums[-1], error_bound(ip, ix, dt, x0, rhs), True)
    assert res.error > 0.0


def test_contract_violations(hip):
    """heat.rs:109-110 asserts, heat.rs:127 diag.unwrap(), CSC operand, aliasing, mixed precision, n = 0"""
    import ctypes as C
    from sprs_amd import _ffi
    from sprs_amd.device import DeviceCsMat, DeviceCsMatF32, DeviceVec, DeviceVecF32, CSC
    from sprs_amd.linalg import gauss_seidel
    shape, ip, ix, dt, rhs = heat32(6)
    a = DeviceCsMatF32.from_host(shape, ip, ix, dt)
    with pytest.raises(_ffi.SprsHipError) as e:
        gauss_seidel(a, DeviceVecF32.zeros(35), DeviceVecF32.zeros(35), 3, 1e-8)
    assert e.value.status == _ffi.DIM_MISMATCH
    csc = DeviceCsMatF32.from_host(shape, ip, ix, dt, storage=CSC)
    with pytest.raises(_ffi.SprsHipError) as e:
        gauss_seidel(csc, DeviceVecF32.zeros(36), DeviceVecF32.zeros(36), 3, 1e-8)
    assert e.value.status == _ffi.STORAGE_MISMATCH
    # a row without a diagonal entry: the reference panics in the first sweep; with no sweep asked for it does not
    nd_ip = np.array([0, 1, 2, 3], dtype=np.uint64)
    nd_ix = np.array([0, 0, 2], dtype=np.uint64)
    nd = DeviceCsMatF32.from_host((3, 3), nd_ip, nd_ix, np.ones(3, dtype=np.float32))
    with pytest.raises(_ffi.SprsHipError) as e:
        gauss_seidel(nd, DeviceVecF32.zeros(3), DeviceVecF32.zeros(3), 1, 1e-8)
    assert e.value.status == _ffi.BAD_STRUCTURE and "row 1" in str(e.value)
    with pytest.raises(ref.NoDiagonal):
        ref.gauss_seidel((3, 3), nd_ip, nd_ix, np.ones(3, dtype=np.float32), np.zeros(3, dtype=np.float32), np.zeros(3, dtype=np.float32), 1, 1e-8)
    res = gauss_seidel(nd, DeviceVecF32.zeros(3), DeviceVecF32.zeros(3), 0, 1e-8)
    assert not res.converged and res.error == 0.0
    # x aliasing rhs
    v = DeviceVecF32.zeros(36)
    info = C.create_string_buffer(64)
    assert _ffi.lib.sprs_hip_gauss_seidel_f32(a._h, C.c_void_p(v.ptr), C.c_void_p(v.ptr), 36, 1, 1e-8, info, None) == _ffi.INVALID_ARG
    with pytest.raises(_ffi.SprsHipError) as e:
        gauss_seidel(a, v, v, 1, 1e-8)
    assert e.value.status == _ffi.INVALID_ARG and "alias" in str(e.value)
    # mixed precision: never reaches the library
    with pytest.raises(TypeError):
        gauss_seidel(a, DeviceVec.zeros(36), DeviceVecF32.zeros(36), 1, 1e-8)
    with pytest.raises(TypeError):
        gauss_seidel(a, DeviceVecF32.zeros(36), DeviceVec.zeros(36), 1, 1e-8)
    s64 = heat_system(6)
    with pytest.raises(TypeError):
        gauss_seidel(DeviceCsMat.from_host(*s64[:4]), DeviceVecF32.zeros(36), DeviceVecF32.zeros(36), 1, 1e-8)
    # n == 0: the empty sum is 0 < eps
    empty = DeviceCsMatF32.from_host((0, 0), np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.float32))
    res = gauss_seidel(empty, DeviceVecF32(0), DeviceVecF32(0), 5, 1e-8)
    assert res.converged and res.iterations == 0 and res.error == 0.0


def test_band_schedule_is_f64_only(hip):
    """option gauss_seidel_chain = S: INVALID_ARG with a text that says so on an f32 handle; the option is restored"""
    rows = 64
    shape, ip, ix, dt, rhs = heat32(rows)
    x0 = np.zeros(rows * rows, dtype=np.float32)
    hip.set_option("gauss_seidel_chain", rows)
    try:
        with pytest.raises(hip.SprsHipError) as e:
            gpu_gs(shape, ip, ix, dt, x0, rhs, 1, -1.0)
        assert e.value.status == hip._ffi.INVALID_ARG and "f64" in str(e.value) and "gauss_seidel_chain" in str(e.value)
    finally:
        hip.set_option("gauss_seidel_chain", 0)
    x, res = gpu_gs(shape, ip, ix, dt, x0, rhs, 1, -1.0)       # and with the option back at 0 the sweep runs
    assert res.iterations == 1 and np.isfinite(x).all()


class _Wrapped32:
    """three raw device buffers behind sprs_hip_csmat_f32_wrap_device: a handle whose values the test can change in place"""

    def __init__(self, storage, n, ip, ix, dt):
        import ctypes as C
        from sprs_amd import _ffi
        from sprs_amd.device import DeviceCsMatF32
        self.lib, self.bufs = _ffi.lib, []
        ptrs = [self._upload(arr) for arr in (ip.astype(np.uint64), ix.astype(np.uint64), dt.astype(np.float32))]
        h = C.c_void_p()
        _ffi.check(self.lib.sprs_hip_csmat_f32_wrap_device(C.byref(h), storage, n, n, ix.size, ptrs[0], 8, ptrs[1], 8, ptrs[2]))
        self.mat = DeviceCsMatF32(h.value, keep=self)
        self.data = ptrs[2]

    def _upload(self, arr):
        import ctypes as C
        from sprs_amd import _ffi
        arr = np.ascontiguousarray(arr)
        p = C.c_void_p()
        _ffi.check(self.lib.sprs_hip_malloc(C.byref(p), max(arr.nbytes, 8)))
        self.bufs.append(p)
        _ffi.check(self.lib.sprs_hip_memcpy_h2d(p, C.c_void_p(arr.ctypes.data), arr.nbytes))
        return p

    def set_values(self, dt):
        import ctypes as C
        from sprs_amd import _ffi
        dt = np.ascontiguousarray(dt, dtype=np.float32)
        _ffi.check(self.lib.sprs_hip_memcpy_h2d(self.data, C.c_void_p(dt.ctypes.data), dt.nbytes))
        self.mat.refresh()

    def free(self):
        self.mat = None
        for p in self.bufs:
            self.lib.sprs_hip_free(p)
        self.bufs = []


@pytest.mark.parametrize("storage", ["csr", "csc"])
def test_plans_follow_refresh(hip, storage):
    """a triangular solve and a sweep on one handle (both level plans and, for CSC, the cached CSR form), then new values of the
    same structure + refresh: the new values' results, bit for bit"""
    from sprs_amd.device import DeviceVecF32, CSC, CSR
    from sprs_amd import linalg
    n = 150
    a = _random_system(n, 21, 4)
    rng = np.random.default_rng(4)
    b, x0 = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    m = a.tocsc() if storage == "csc" else a.tocsr()
    m.sort_indices()
    ip, ix = m.indptr.astype(np.uint64), m.indices.astype(np.uint64)
    csr = a.tocsr()
    csr.sort_indices()
    rip, rix = csr.indptr.astype(np.uint64), csr.indices.astype(np.uint64)
    w = _Wrapped32(CSC if storage == "csc" else CSR, n, ip, ix, m.data)
    try:
        for scale in (None, np.random.default_rng(2).uniform(1.0, 1.01, a.nnz)):
            if scale is not None:
                a = a.copy()
                a.data = a.data * scale                       # still strictly diagonally dominant
                m = a.tocsc() if storage == "csc" else a.tocsr()
                m.sort_indices()
                w.set_values(m.data)
            dt = m.data.astype(np.float32)
            for kind in ("lsolve", "usolve"):
                x = DeviceVecF32.from_host(b)
                res = getattr(linalg, "%s_%s_dense_rhs" % (kind, storage))(w.mat, x)
                assert np.array_equal(x.to_host(), ref.SOLVES[kind + "_" + storage](n, ip, ix, dt, b))
                assert res.levels == ref.levels(kind + "_" + storage, n, ip, ix)
            if storage == "csr":
                csr = a.tocsr()
                csr.sort_indices()
                want = ref.gauss_seidel((n, n), rip, rix, csr.data.astype(np.float32), x0, b, 2, -1.0)
                x = DeviceVecF32.from_host(x0)
                res = linalg.gauss_seidel(w.mat, x, DeviceVecF32.from_host(b), 2, -1.0)
                assert np.array_equal(x.to_host(), want.x)
                assert res.levels == ref.levels("lsolve_csr", n, rip, rix)
    finally:
        w.free()
