"""The restatement tests/ldl_ref.py against the reference's own golden vectors (tests/golden/ldl_fixtures.json, extracted from
sprs-ldl/src/lib.rs:634-866) and its two formulations against each other.  No device: this pins the oracle that
tests/test_ldl_gpu.py compares the kernels with.  Every comparison is exact equality of integers or of value bits."""
import json
import os

import numpy as np
import pytest

import ldl_ref as R
from conftest import ROOT

DENSITIES = (0.05, 0.15, 0.3, 0.6)
SIZES = (2, 3, 5, 9, 17, 33, 60)


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(ROOT, "tests", "golden", "ldl_fixtures.json")) as f:
        return json.load(f)


def _same_bits(got, want):
    return np.array_equal(R.bits(got), R.bits(want))


def _mat(m):
    return m["shape"][0], m["indptr"], m["indices"], m["data"]


@pytest.mark.parametrize("closed", [False, True])
def test_restatement_reproduces_the_golden_factors(fx, closed):
    """test_factor1 (lib.rs:732-778)"""
    parents, colptr, l_indices, l_data, d = R.factor(*_mat(fx["mat1"]), None, closed=closed)
    f = fx["factors1"]
    assert colptr == f["colptr"] and l_indices == f["indices"]
    assert _same_bits(l_data, f["data"]) and _same_bits(d, f["d"])
    assert parents == [8, 4, None, None, 6, None, 7, 8, 9, None]


def test_restatement_reproduces_the_golden_solves(fx):
    """test_solve1 and test_factor_solve1 (lib.rs:780-811)"""
    f = fx["factors1"]
    x, stages = R.solve(10, f["colptr"], f["indices"], f["data"], f["d"], None, fx["vec1"])
    assert _same_bits(stages[0], fx["lsolve1"]) and _same_bits(stages[1], fx["dsolve1"]) and _same_bits(stages[2], fx["res1"])
    assert _same_bits(x, fx["res1"])
    _, colptr, l_indices, l_data, d = R.factor(*_mat(fx["mat1"]))
    assert _same_bits(R.solve(10, colptr, l_indices, l_data, d, None, fx["vec1"])[0], fx["res1"])


def test_permuted_system(fx):
    """permuted_ldl_solve (lib.rs:814-845): L, D and the solution of the comment's picture"""
    p = fx["permuted"]
    parents, colptr, l_indices, l_data, d = R.factor(*_mat(p), p["perm"])
    assert (parents, colptr, l_indices, l_data, d) == ([3, 2, None, None], [0, 1, 2, 2, 2], [3, 2], [2.0, 3.0], [1.0, 2.0, 3.0, 4.0])
    assert R.solve(4, colptr, l_indices, l_data, d, p["perm"], p["b"])[0] == p["x"] == [1.0, 2.0, 3.0, 4.0]


def _cases():
    for n in SIZES:
        for density in DENSITIES:
            for seed in range(3):
                m = R.random_symmetric(n, density, 100 * seed + n)
                yield m, None
                yield m, np.random.RandomState(seed + n).permutation(n).tolist()


def test_formulations_agree_and_the_order_matters():
    """The sequential loop and the closed form give the same bits on random symmetric matrices (n from 2 to 60, four densities,
    identity and random permutations); walking the patterns by ascending index instead does NOT, in a good share of them — so
    a kernel that ignored the order would be caught by the cases the GPU tests draw from this generator."""
    total = sensitive = unordered = 0
    for m, perm in _cases():
        a = R.factor(*m, perm)
        b = R.factor(*m, perm, closed=True)
        assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2]
        assert _same_bits(a[3], b[3]) and _same_bits(a[4], b[4])
        n = m[0]
        rows = R.row_patterns(n, m[1], m[2], perm, a[0])
        unordered += any(sorted(r, key=lambda i: (-r[i], i)) != sorted(r) for r in rows)
        asc = R.numeric_closed(*m, perm, a[1], a[0], ascending=True)
        assert asc[0] == a[2]                                   # the structure does not depend on the order
        total += 1
        sensitive += not (_same_bits(asc[1], a[3]) and _same_bits(asc[2], a[4]))
    assert total == 2 * 3 * len(SIZES) * len(DENSITIES)
    assert unordered >= total // 4, (unordered, total)
    assert sensitive >= total // 8, (sensitive, total)


def test_gpu_cases_are_order_sensitive():
    """the four generator settings tests/test_ldl_gpu.py::test_order_sensitive_cases uses"""
    hit = 0
    for n, density, seed in ((17, 0.3, 7), (33, 0.15, 8), (60, 0.15, 9), (60, 0.3, 10)):
        m = R.random_symmetric(n, density, seed)
        for perm in (None, np.random.RandomState(seed).permutation(n).tolist()):
            a = R.factor(*m, perm)
            asc = R.numeric_closed(*m, perm, a[1], a[0], ascending=True)
            hit += not (_same_bits(asc[1], a[3]) and _same_bits(asc[2], a[4]))
    assert hit >= 2


def test_singular_and_symbolic_edges():
    for dense, index in (([[1.0, 1.0], [1.0, 1.0]], 1), ([[0.0, 1.0], [1.0, 1.0]], 0)):
        m = R.dense_to_cs(np.array(dense), keep_diagonal=True)
        for closed in (False, True):
            with pytest.raises(R.Singular) as e:
                R.factor(*m, None, closed=closed)
            assert e.value.index == index
    m = R.dense_to_cs(np.array([[2.0, 0, 0, 0], [0, 0.0, 1.0, 0], [0, 1.0, 3.0, 0], [0, 0, 0, 0.0]]), keep_diagonal=True)
    parents, _, colptr = R.symbolic(m[0], m[1], m[2])
    *_, first = R.numeric_closed(*m, None, colptr, parents, stop_at_singular=False)
    assert first == 1                                           # two zero pivots: the smaller index
    assert R.symbolic(1, [0, 1], [0]) == ([None], [0], [0, 0])
