"""Pins tests/f32_solve_ref.py, the np.float32 restatement the f32 GPU tests compare with: the reference's golden systems, the
f64 restatement within the f32 rounding bound, its own CSR and CSC forms where their orders coincide, and the f32-specific
properties the GPU tests rely on (results are float32, every step rounds once, the singular returns)."""
import json
import os

import numpy as np
import pytest

import f32_solve_ref as ref
import trisolve_ref as ref64

F = np.float32
U = 2.0 ** -24
KINDS = ["lsolve_csr", "usolve_csr", "lsolve_csc", "usolve_csc"]


def _system(n, seed, per_row=4):
    """scipy CSR: non-symmetric, strictly diagonally dominant (well conditioned triangles), sorted rows"""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    r = np.repeat(np.arange(n), per_row)
    c = rng.integers(0, n, size=r.size)
    a = sp.coo_matrix((rng.standard_normal(r.size), (r, c)), shape=(n, n)).tocsr()
    a = (a + sp.diags(np.abs(a).sum(axis=1).A1 + 1.0 + rng.random(n))).tocsr()
    a.sort_indices()
    return a


def _arrays(a, kind):
    m = a.tocsc() if kind.endswith("csc") else a.tocsr()
    m.sort_indices()
    return m.indptr.astype(np.uint64), m.indices.astype(np.uint64), m.data.astype(np.float32)


def test_golden_systems():
    """the reference's own unit tests (trisolve.rs:368-442): small integers and halves, exact in f32"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trisolve_fixtures.json")
    systems = json.load(open(path))["systems"]
    assert sorted(s["solve"] for s in systems) == sorted(KINDS)
    for s in systems:
        ip, ix = np.array(s["indptr"], dtype=np.uint64), np.array(s["indices"], dtype=np.uint64)
        x = ref.SOLVES[s["solve"]](s["shape"][0], ip, ix, np.array(s["data"], dtype=np.float32), np.array(s["b"], dtype=np.float32))
        assert x.dtype == np.float32
        assert np.array_equal(x, np.array(s["x"], dtype=np.float32)), s["solve"]


@pytest.mark.parametrize("kind", KINDS)
def test_agrees_with_the_f64_restatement(kind):
    """the same f32-valued system solved in f64: a row of m entries takes m + 1 roundings of relative size u on top of those its
    operands carry, n rows deep at the most — n m u relative to the largest unknown on a strictly diagonally dominant system
    (errors are damped, not amplified, from row to row)"""
    n = 120
    a = _system(n, 5)
    ip, ix, dt = _arrays(a, kind)
    b = np.random.default_rng(6).standard_normal(n).astype(np.float32)
    x32 = ref.SOLVES[kind](n, ip, ix, dt, b)
    x64 = ref64.SOLVES[kind](n, ip, ix, dt.astype(np.float64), b.astype(np.float64))
    m = int(np.diff(ip.astype(np.int64)).max())
    assert x32.dtype == np.float32
    assert np.abs(x32.astype(np.float64) - x64).max() <= n * m * U * np.abs(x64).max()
    assert not np.array_equal(x32, x64.astype(np.float32))          # and it is not the f64 solve rounded at the end


@pytest.mark.parametrize("seed", [1, 2])
def test_lower_csr_and_csc_forms_coincide(seed):
    """lsolve_csc scatters column by column, ascending: row r receives its products by ascending column, which is the stored
    order of a sorted CSR row — the two lower solves give the same bits.  The upper ones do not (usolve_csc: descending)"""
    n = 90
    a = _system(n, seed)
    b = np.random.default_rng(seed + 10).standard_normal(n).astype(np.float32)
    got = {kind: ref.SOLVES[kind](n, *_arrays(a, kind), b) for kind in KINDS}
    assert np.array_equal(got["lsolve_csr"], got["lsolve_csc"])
    assert not np.array_equal(got["usolve_csr"], got["usolve_csc"])
    assert np.allclose(got["usolve_csr"], got["usolve_csc"], rtol=0, atol=1e-4)


def test_singular_returns():
    """index and reason as tests/trisolve_ref.py has them: -0.0f counts as zero, NaN does not, a missing diagonal is structural on
    CSC and "is 0" / "numeric" on CSR"""
    ip = np.array([0, 1, 3, 5], dtype=np.uint64)
    ix = np.array([0, 0, 1, 1, 2], dtype=np.uint64)
    b = np.ones(3, dtype=np.float32)
    for zero in (F(0.0), F(-0.0)):
        dt = np.array([2.0, 1.0, zero, 1.0, 4.0], dtype=np.float32)
        with pytest.raises(ref.Singular) as e:
            ref.lsolve_csr_dense_rhs(3, ip, ix, dt, b)
        assert (e.value.index, e.value.reason) == (1, "diagonal element is 0")
        with pytest.raises(ref.Singular) as e:
            ref.usolve_csr_dense_rhs(3, ip, ix, dt, b)
        assert (e.value.index, e.value.reason) == (1, "diagonal element is a numeric 0")
    dt = np.array([2.0, 1.0, np.nan, 1.0, 4.0], dtype=np.float32)
    x = ref.lsolve_csr_dense_rhs(3, ip, ix, dt, b)
    assert np.isnan(x[1]) and np.isnan(x[2]) and x[0] == F(0.5)
    # the same arrays read as CSC: column 1 = rows {0, 1}; without its diagonal the CSC solves call it structural
    cip = np.array([0, 1, 2, 3], dtype=np.uint64)
    cix = np.array([0, 0, 2], dtype=np.uint64)
    cdt = np.ones(3, dtype=np.float32)
    for kind in ("lsolve_csc", "usolve_csc"):
        with pytest.raises(ref.Singular) as e:
            ref.SOLVES[kind](3, cip, cix, cdt, b)
        assert (e.value.index, e.value.reason) == (1, "diagonal element is a structural 0")
    with pytest.raises(ref.Singular) as e:
        ref.lsolve_csr_dense_rhs(3, cip, cix, cdt, b)
    assert (e.value.index, e.value.reason) == (1, "diagonal element is 0")


def test_every_step_rounds_once():
    """1 - 0.6f * x with x = fl(1/3): two f32 operations give other bits than the exact product subtracted and rounded once"""
    ip = np.array([0, 1, 3], dtype=np.uint64)
    ix = np.array([0, 0, 1], dtype=np.uint64)
    dt = np.array([3.0, 0.6, 1.0], dtype=np.float32)
    x = ref.lsolve_csr_dense_rhs(2, ip, ix, dt, np.ones(2, dtype=np.float32))
    assert x[0] == F(F(1.0) / F(3.0))
    assert x[1] == F(F(1.0) - F(dt[1] * x[0]))
    assert x[1] != F(1.0 - float(dt[1]) * float(x[0]))


def test_gauss_seidel_restatement():
    """heat.rs:103-139 in f32 on a 2 x 2 system worked by hand, the Ok / Err returns, max_iter = 0, the row without a diagonal"""
    ip = np.array([0, 2, 4], dtype=np.uint64)
    ix = np.array([0, 1, 0, 1], dtype=np.uint64)
    dt = np.array([4.0, 1.0, 2.0, 5.0], dtype=np.float32)
    rhs = np.array([1.0, 2.0], dtype=np.float32)
    x0 = np.zeros(2, dtype=np.float32)
    r = ref.gauss_seidel((2, 2), ip, ix, dt, x0, rhs, 1, -1.0)
    x_0 = F(F(1.0) - F(0.0)) / F(4.0)
    x_1 = F(F(2.0) - F(F(2.0) * x_0)) / F(5.0)
    assert r.x.dtype == np.float32 and np.array_equal(r.x, np.array([x_0, x_1], dtype=np.float32))
    assert (r.iterations, r.converged) == (1, False) and len(r.sums) == 2
    # the scalar: (A x - rhs).sum().sqrt() of the LAST iterate, in f32; the start vector's is sqrt(-3) = NaN
    v = np.array([F(F(4.0) * x_0) + F(F(1.0) * x_1), F(F(2.0) * x_0) + F(F(5.0) * x_1)], dtype=np.float32)
    assert r.sums[1] == F(F(v[0] - rhs[0]) + F(v[1] - rhs[1])) and np.isnan(r.errors[0])
    assert (np.isnan(r.error) and r.sums[1] < 0) or r.error == F(np.sqrt(r.sums[1]))
    zero = ref.gauss_seidel((2, 2), ip, ix, dt, np.ones(2, dtype=np.float32), rhs, 0, 1e-3)
    assert np.array_equal(zero.x, np.ones(2, dtype=np.float32)) and (zero.iterations, zero.converged) == (0, False)
    assert zero.error == F(3.0)                                   # sqrt((5 - 1) + (7 - 2))
    ok = ref.gauss_seidel((2, 2), ip, ix, dt, np.ones(2, dtype=np.float32), rhs, 50, 10.0)
    first = next(i for i, e in enumerate(ok.errors[1:]) if e < F(10.0))       # (a NaN is below nothing)
    assert ok.converged and ok.iterations == first and ok.error == ok.errors[first + 1]
    with pytest.raises(ref.NoDiagonal):
        ref.gauss_seidel((2, 2), np.array([0, 1, 2], dtype=np.uint64), np.array([0, 0], dtype=np.uint64), np.ones(2, dtype=np.float32),
                         x0, rhs, 1, 1e-3)


def test_ndarray_sum_order():
    """eight interleaved partial sums over the full blocks of eight, combined as (p0+p4), (p1+p5), (p2+p6), (p3+p7) in turn, then
    the tail one by one — on values where the order shows in f32"""
    xs = np.array([2.0 ** 24, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, -(2.0 ** 24), 1.0], dtype=np.float32)
    want = F(0.0)
    for k in range(4):                                        # one full block: p_k = xs[k]
        want = F(want + F(xs[k] + xs[k + 4]))
    for v in xs[8:]:                                          # fewer than eight left: one by one
        want = F(want + v)
    left_to_right = F(0.0)
    for v in xs:
        left_to_right = F(left_to_right + v)
    assert ref.ndarray_sum(xs) == want and want != left_to_right
    assert ref.ndarray_sum(np.zeros(0, dtype=np.float32)) == F(0.0)
    assert ref.ndarray_sum(np.arange(16, dtype=np.float32)) == F(120.0)
