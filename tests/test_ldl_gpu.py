"""Device LDL^T — Ldl, LdlSymbolic, LdlNumeric, ldl_lsolve / ldl_ltsolve / diag_solve (sprs-ldl/src/lib.rs) — against the golden
vectors of the reference's own tests and the restatement tests/ldl_ref.py.  Every comparison is exact: integers, or the bits of
f64 values; there is no tolerance anywhere.

The small cases also run against the kernel emulator (tests/test_ldl_emu_cpu.py); the grid and the torch cases need a real device."""
import json
import os

import numpy as np
import pytest

import ldl_ref as R
from conftest import IDX_COMBOS, ROOT

pytestmark = pytest.mark.gpu

EMULATED = bool(os.environ.get("SPRS_HIP_LIBRARY"))
CSR, CSC = 0, 1
NONE = 2**64 - 1


@pytest.fixture(scope="module", autouse=True)
def _need_device():
    import sprs_amd
    if sprs_amd.device_count() < 1:
        pytest.skip("no HIP device")


@pytest.fixture(autouse=True)
def _default_options():
    import sprs_amd
    yield
    sprs_amd.set_option("ldl_lds_cap", 1024)


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(ROOT, "tests", "golden", "ldl_fixtures.json")) as f:
        return json.load(f)


def _fixture_mat(m):
    return m["shape"][0], np.array(m["indptr"], dtype=np.uint64), np.array(m["indices"], dtype=np.uint64), np.array(m["data"], dtype=np.float64)


def _mat(m, storage=CSC, idx=np.uint64, ptr=np.uint64):
    from sprs_amd.device import DeviceCsMat
    n, ip, ix, dt = m
    return DeviceCsMat.from_host((n, n), np.asarray(ip).astype(ptr), np.asarray(ix).astype(idx), np.asarray(dt, dtype=np.float64), storage=storage)


def _perm(perm, idx=np.uint64):
    from sprs_amd import DevicePerm
    return None if perm is None else DevicePerm(np.asarray(perm, dtype=idx))


def _same_bits(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))


def _same_factors(sym, num, ref):
    parents, colptr, l_indices, l_data, d = ref
    n = len(parents)
    assert sym.problem_size() == n and sym.nnz() == colptr[n] and num.problem_size() == n and num.nnz() == colptr[n]
    assert sym.colptr().tolist() == colptr
    assert sym.parents() == parents
    shape, ip, ix, dt = num.l().to_host()
    assert tuple(shape) == (n, n) and num.l().is_csc()
    assert ip.tolist() == colptr and ix.tolist() == l_indices
    assert _same_bits(dt, l_data)
    assert _same_bits(num.d().to_host(), d)


def _rhs(n, seed):
    return np.random.RandomState(seed).standard_normal(n) * 7.0 + 0.25


def _check(m, perm=None, storage=CSC, idx=np.uint64, ptr=np.uint64, check_symmetry=True, cap=None, seed=5):
    """symbolic, factor and solve of m under perm against the restatement; returns (sym, num, a, ref)"""
    import sprs_amd
    from sprs_amd import LdlSymbolic
    from sprs_amd.device import DeviceVec
    if cap is not None:
        sprs_amd.set_option("ldl_lds_cap", cap)
    n = m[0]
    ref = R.factor(*m, perm)
    a = _mat(m, storage, idx, ptr)
    sym = LdlSymbolic.new_perm(a, _perm(perm, idx), check_symmetry)
    num = sym.factor(a)
    _same_factors(sym, num, ref)
    b = _rhs(n, seed)
    x = num.solve(DeviceVec.from_host(b)).to_host()
    want, _ = R.solve(n, ref[1], ref[2], ref[3], ref[4], perm, b)
    assert _same_bits(x, want)
    return sym, num, a, ref


# ---- 1. the golden 10 x 10 system (lib.rs:634-811) -------------------------------------------------------------------------

def test_golden_factor(fx):
    from sprs_amd import LdlSymbolic
    m = _fixture_mat(fx["mat1"])
    a = _mat(m)
    sym = LdlSymbolic.new(a)
    num = sym.factor(a)
    f = fx["factors1"]
    assert sym.colptr().tolist() == f["colptr"]
    _, ip, ix, dt = num.l().to_host()
    assert ip.tolist() == f["colptr"] and ix.tolist() == f["indices"]
    assert _same_bits(dt, f["data"])
    assert _same_bits(num.d().to_host(), f["d"])


def test_golden_solve_stages(fx):
    """test_solve1: ldl_lsolve, diag_solve, ldl_ltsolve through the free functions, on the expected factors"""
    from sprs_amd import diag_solve, ldl_lsolve, ldl_ltsolve
    from sprs_amd.device import DeviceCsMat, DeviceVec
    f = fx["factors1"]
    for idx, ptr in IDX_COMBOS:
        l = DeviceCsMat.from_host((10, 10), np.array(f["colptr"], dtype=ptr), np.array(f["indices"], dtype=idx), np.array(f["data"]), storage=CSC)
        x = DeviceVec.from_host(np.array(fx["vec1"]))
        ldl_lsolve(l, x)
        assert _same_bits(x.to_host(), fx["lsolve1"])
        diag_solve(DeviceVec.from_host(np.array(f["d"])), x)
        assert _same_bits(x.to_host(), fx["dsolve1"])
        ldl_ltsolve(l, x)
        assert _same_bits(x.to_host(), fx["res1"])
        ldl_ltsolve(l, x)                                   # the cached row order serves a second call
        ldl_lsolve(l, x)


def test_golden_factor_solve(fx):
    """test_factor_solve1: LdlNumeric::new end to end"""
    from sprs_amd import LdlNumeric
    from sprs_amd.device import DeviceVec
    for storage in (CSC, CSR):
        num = LdlNumeric.new(_mat(_fixture_mat(fx["mat1"]), storage))
        assert _same_bits(num.solve(DeviceVec.from_host(np.array(fx["vec1"]))).to_host(), fx["res1"])


# ---- 2. the permuted 4 x 4 system (lib.rs:814-866) --------------------------------------------------------------------------

def test_permuted_solve(fx):
    from sprs_amd.device import DeviceVec
    p = fx["permuted"]
    sym, num, a, ref = _check(_fixture_mat(p), p["perm"])
    assert num.solve(DeviceVec.from_host(np.array(p["b"]))).to_host().tolist() == [1.0, 2.0, 3.0, 4.0]
    assert sym.perm().vec().tolist() == p["perm"]


def test_cuthill_solve(fx):
    from sprs_amd import FillInReduction, Ldl, SymmetryCheck
    from sprs_amd.device import DeviceVec
    p = fx["permuted"]
    m = _fixture_mat(p)
    a = _mat(m)
    builder = Ldl.new().check_symmetry(SymmetryCheck.DontCheckSymmetry).fill_in_reduction(FillInReduction.ReverseCuthillMcKee)
    sym = builder.symbolic(a)
    num = sym.factor(a)
    assert num.solve(DeviceVec.from_host(np.array(p["b"]))).to_host().tolist() == [1.0, 2.0, 3.0, 4.0]
    perm = sym.perm().vec().tolist()
    assert sorted(perm) == [0, 1, 2, 3]
    _same_factors(sym, num, R.factor(*m, perm))
    assert builder.numeric(a).solve(DeviceVec.from_host(np.array(p["b"]))).to_host().tolist() == [1.0, 2.0, 3.0, 4.0]
    assert Ldl().check_perm(False).fill_in_reduction(FillInReduction.NoReduction).perm(a) is None


# ---- 3. random diagonally dominant symmetric matrices ------------------------------------------------------------------------

def _random_case(n, seed):
    density = {2: 1.0, 3: 0.7}.get(n, min(0.5, 6.0 / n))
    return R.random_symmetric(n, density, seed)


@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 200])
def test_random(n):
    from sprs_amd import reverse_cuthill_mckee
    m = _random_case(n, 1000 + n)
    rnd = np.random.RandomState(n).permutation(n).tolist()
    rcm = reverse_cuthill_mckee(_mat(m)).perm.vec().tolist()
    k = 0
    for perm in (None, rnd, rcm):
        for idx, ptr in IDX_COMBOS:
            _check(m, perm, (CSR, CSC)[k % 2], idx, ptr, seed=n + k)
            k += 1
        _check(m, perm, (CSR, CSC)[k % 2], seed=n + k)      # both storages meet every kind of permutation


def test_order_sensitive_cases():
    """cases of tests/test_ldl_cpu.py whose bits change when a pattern is walked by ascending index"""
    hit = 0
    for n, density, seed in ((17, 0.3, 7), (33, 0.15, 8), (60, 0.15, 9), (60, 0.3, 10)):
        m = R.random_symmetric(n, density, seed)
        for perm in (None, np.random.RandomState(seed).permutation(n).tolist()):
            _, _, _, ref = _check(m, perm, (CSR, CSC)[hit % 2])
            asc = R.numeric_closed(*m, perm, ref[1], ref[0], ascending=True)
            hit += not (_same_bits(asc[1], ref[3]) and _same_bits(asc[2], ref[4]))
    assert hit >= 2, "no case here can tell the reference's order from the ascending one"


# ---- 4. seams ------------------------------------------------------------------------------------------------------------------

def _dense_case(a):
    return R.dense_to_cs(np.asarray(a, dtype=np.float64))


def test_diagonal_matrix():
    sym, num, _, _ = _check(_dense_case(np.diag([2.0, -3.0, 0.5, 7.0, 1.25])))
    assert sym.nnz() == 0 and sym.parents() == [None] * 5


def test_block_diagonal_forest():
    rng = np.random.RandomState(3)
    a = np.zeros((200, 200))
    for b in range(40):
        blk = rng.standard_normal((5, 5)) * (rng.rand(5, 5) < 0.6)
        blk = blk + blk.T + np.diag(20.0 + rng.rand(5))
        a[5 * b:5 * b + 5, 5 * b:5 * b + 5] = blk
    sym, _, _, _ = _check(_dense_case(a))
    assert sym.parents().count(None) >= 40
    _check(_dense_case(a), np.random.RandomState(4).permutation(200).tolist(), CSR, np.uint32, np.uint32)


def test_tridiagonal_chain():
    n = 257
    rng = np.random.RandomState(11)
    off = rng.standard_normal(n - 1)
    a = np.diag(3.0 + rng.rand(n)) + np.diag(off, 1) + np.diag(off, -1)
    sym, _, _, _ = _check(_dense_case(a))
    assert sym.parents() == list(range(1, n)) + [None]


def test_dense_matrix():
    n = 70
    rng = np.random.RandomState(12)
    a = rng.standard_normal((n, n))
    a = a + a.T + np.diag(2.0 * n + rng.rand(n))
    sym, _, _, _ = _check(_dense_case(a))
    assert sym.nnz() == n * (n - 1) // 2
    _check(_dense_case(a), list(range(n - 1, -1, -1)), CSR, cap=8)


def _arrow(n, hub):
    rng = np.random.RandomState(13 + hub)
    a = np.diag(4.0 + rng.rand(n))
    v = rng.standard_normal(n) * 0.05
    a[hub, :] = v
    a[:, hub] = v
    a[hub, hub] = 9.0
    return _dense_case(a)


@pytest.mark.parametrize("cap", [1024, 8])
def test_arrow_matrix(cap):
    n = 300
    sym, _, _, _ = _check(_arrow(n, n - 1), cap=cap)              # hub last: no fill
    assert sym.nnz() == n - 1
    sym, _, _, _ = _check(_arrow(n, n - 1), list(range(n - 1, -1, -1)), CSR, np.uint32, np.uint64, cap=cap)   # hub first: a dense L
    assert sym.nnz() == n * (n - 1) // 2


def test_row_without_stored_diagonal():
    a = np.array([[4.0, 1.0, 0.0, 2.0], [1.0, 0.0, 3.0, 0.0], [0.0, 3.0, 5.0, 1.0], [2.0, 0.0, 1.0, 6.0]])
    m = _dense_case(a)
    assert 1 not in m[2][int(m[1][1]):int(m[1][2])]               # row 1 stores no diagonal: d[1] starts from 0
    _check(m)
    _check(m, [2, 0, 3, 1], CSR)


# ---- 5. update ---------------------------------------------------------------------------------------------------------------

def test_update_and_repeats():
    from sprs_amd.device import DeviceVec
    n = 65
    m = _random_case(n, 77)
    perm = np.random.RandomState(78).permutation(n).tolist()
    sym, num, a, ref = _check(m, perm)
    want_l, want_d = num.l().to_host()[3], num.d().to_host()
    for _ in range(5):                                              # repeated factors are bit-identical
        again = sym.factor(a)
        assert _same_bits(again.l().to_host()[3], want_l) and _same_bits(again.d().to_host(), want_d)
    rng = np.random.RandomState(79)
    dense = np.zeros((n, n))
    for r in range(n):
        for p in range(int(m[1][r]), int(m[1][r + 1])):
            c = int(m[2][p])
            if c >= r:
                dense[r, c] = dense[c, r] = m[3][p] * (1.0 + 0.25 * rng.rand())
    m2 = (n, m[1], m[2], np.array([dense[r, int(m[2][p])] for r in range(n) for p in range(int(m[1][r]), int(m[1][r + 1]))]))
    a2 = _mat(m2)
    num.update(a2)
    ref2 = R.factor(*m2, perm)
    _same_factors(sym, num, ref2)
    fresh = sym.factor(a2)
    assert _same_bits(fresh.l().to_host()[3], num.l().to_host()[3]) and _same_bits(fresh.d().to_host(), num.d().to_host())
    b = _rhs(n, 80)
    want, _ = R.solve(n, ref2[1], ref2[2], ref2[3], ref2[4], perm, b)
    assert _same_bits(num.solve(DeviceVec.from_host(b)).to_host(), want)      # solve after update uses the new factors
    del sym                                                          # the numeric handle keeps the analysis alive
    num.update(a)
    assert _same_bits(num.d().to_host(), ref[4])


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------

def test_errors():
    import sprs_amd
    from sprs_amd import FillInReduction, Ldl, LdlNumeric, LdlSymbolic, SprsHipError, _ffi
    ns = _dense_case([[4.0, 1.0, 0.0], [2.0, 5.0, 1.0], [0.0, 1.0, 6.0]])          # values differ across the diagonal
    with pytest.raises(SprsHipError) as e:
        LdlSymbolic.new(_mat(ns))
    assert e.value.status == _ffi.BAD_STRUCTURE and "Matrix is not symmetric" in str(e.value)
    ns2 = _dense_case([[4.0, 1.0, 0.0, 1.0], [0.0, 5.0, 1.0, 0.0], [2.0, 1.0, 6.0, 0.0], [0.0, 3.0, 1.0, 7.0]])   # the pattern too
    for m in (ns, ns2):
        for storage in (CSR, CSC):
            _check(m, None, storage, check_symmetry=False)
            _check(m, [1, 2, 0, 3][:m[0]] if m[0] == 4 else [2, 0, 1], storage, check_symmetry=False)
    for dense, index in (([[1.0, 1.0], [1.0, 1.0]], 1), ([[0.0, 1.0], [1.0, 1.0]], 0),
                         ([[2.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 1.0, 3.0, 0.0], [0.0, 0.0, 0.0, 0.0]], 1)):
        m = R.dense_to_cs(np.array(dense), keep_diagonal=True)
        with pytest.raises(SprsHipError) as e:
            LdlNumeric.new(_mat(m))
        assert e.value.status == _ffi.SINGULAR_MATRIX and e.value.index == index and e.value.reason == "numeric"
        assert "Singular matrix at index %d (diagonal element is a numeric 0)" % index in str(e.value)
        with pytest.raises(R.Singular) as r:
            R.factor(*m)
        assert r.value.index == index
    one = R.dense_to_cs(np.array([[3.0]]))
    s1 = LdlSymbolic.new(_mat(one))                                     # symbolic accepts n = 1 ...
    assert s1.problem_size() == 1 and s1.nnz() == 0 and s1.colptr().tolist() == [0, 0]
    with pytest.raises(SprsHipError) as e:                              # ... factor does not: DStack::with_capacity asserts n > 1
        s1.factor(_mat(one))
    assert e.value.status == _ffi.INVALID_ARG and "n > 1" in str(e.value)
    m = _random_case(5, 1)
    with pytest.raises(SprsHipError) as e:
        LdlSymbolic.new_perm(_mat(m), _perm([0, 1, 2, 3]))
    assert e.value.status == _ffi.DIM_MISMATCH
    from sprs_amd.device import DeviceCsMat
    rect = DeviceCsMat.from_host((2, 3), np.array([0, 1, 2], dtype=np.uint64), np.array([0, 1], dtype=np.uint64), np.ones(2))
    with pytest.raises(SprsHipError) as e:
        LdlSymbolic.new_perm(rect, None, False)
    assert e.value.status == _ffi.DIM_MISMATCH
    with pytest.raises(RuntimeError) as e:
        Ldl().fill_in_reduction(FillInReduction.CAMDSuiteSparse).numeric(_mat(m))
    assert "Unavailable without the `sprs_suitesparse_camd` feature" in str(e.value)
    assert sprs_amd.get_option("ldl_lds_cap") == 1024


# ---- stats: read-backs do not grow with n ------------------------------------------------------------------------------------

def test_readbacks_do_not_grow():
    from sprs_amd import LdlSymbolic
    stats = []
    for n in (64, 200):
        sym = LdlSymbolic.new(_mat(_random_case(n, 1000 + n)))
        stats.append(sym.stats)
    assert stats[0]["readbacks"] == stats[1]["readbacks"] == 2          # is_symmetric's flag and nnz(L)
    assert stats[0]["etree_launches"] == stats[1]["etree_launches"] == 1


# ---- 7. torch tensors on a caller's stream ------------------------------------------------------------------------------------

@pytest.mark.skipif(EMULATED, reason="torch streams: real device only")
def test_solve_on_torch_stream():
    import torch
    from sprs_amd import LdlNumeric
    n = 200
    m = _random_case(n, 1200)
    perm = np.random.RandomState(5).permutation(n).tolist()
    ref = R.factor(*m, perm)
    b = _rhs(n, 6)
    want, _ = R.solve(n, ref[1], ref[2], ref[3], ref[4], perm, b)
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        num = LdlNumeric.new_perm(_mat(m), _perm(perm), True, stream=s)
        rhs = torch.zeros(n, dtype=torch.float64, device=dev)
        out = torch.empty(n, dtype=torch.float64, device=dev)
        torch.cuda._sleep(20_000_000)                      # keep the stream busy: the copy below lands late
        rhs.copy_(torch.from_numpy(b).to(dev, non_blocking=True))
        from sprs_amd.device import DeviceVec
        num.solve(rhs, out=DeviceVec.borrow(out), stream=s)
    s.synchronize()
    assert _same_bits(out.cpu().numpy(), want)


# ---- 8. one larger case on the real device ------------------------------------------------------------------------------------

@pytest.mark.skipif(EMULATED, reason="large case: needs a real device")
def test_grid_laplacian_rcm():
    from sprs_amd import FillInReduction, Ldl
    from sprs_amd.device import DeviceVec
    g = 32
    n = g * g
    indptr, indices, data = [0], [], []
    for r in range(g):
        for c in range(g):
            row = {}
            for dr, dc in ((-1, 0), (0, -1), (0, 0), (0, 1), (1, 0)):
                rr, cc = r + dr, c + dc
                if 0 <= rr < g and 0 <= cc < g:
                    row[rr * g + cc] = 4.5 + 0.001 * ((r * g + c) % 7) if (dr, dc) == (0, 0) else -1.0 - 0.01 * (((r + rr) * 31 + (c + cc) * 17) % 5)
            for k in sorted(row):
                indices.append(k)
                data.append(row[k])
            indptr.append(len(indices))
    m = (n, np.array(indptr, dtype=np.uint64), np.array(indices, dtype=np.uint64), np.array(data))
    a = _mat(m, CSR, np.uint32, np.uint32)
    sym = Ldl().fill_in_reduction(FillInReduction.ReverseCuthillMcKee).symbolic(a)
    num = sym.factor(a)
    perm = sym.perm().vec().tolist()
    ref = R.factor(*m, perm)
    _same_factors(sym, num, ref)
    b = _rhs(n, 9)
    want, _ = R.solve(n, ref[1], ref[2], ref[3], ref[4], perm, b)
    assert _same_bits(num.solve(DeviceVec.from_host(b)).to_host(), want)


@pytest.mark.skipif(EMULATED, reason="links the real library")
def test_cpp_mirror():
    """include/sprs_hip.hpp (namespace ldl) through the same C ABI: the golden system, bit for bit"""
    import subprocess
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = os.path.join(cpp, "ldl_mirror_test.bin")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", cpp, "-f", "ldl_mirror.mk"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all passed" in r.stdout, r.stdout + r.stderr
