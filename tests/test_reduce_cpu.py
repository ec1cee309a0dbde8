"""CPU checks of the yardstick of the sparse-vector reductions: the plain-Python restatement (tests/reduce_ref.py) reproduces the
numbers of the reference's own tests (tests/golden/reduce_fixtures.json), the binary-search dot is the merge dot, the inputs of
the GPU order test really tell the orders apart, and the C entry points refuse bad arguments without a device."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import reduce_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fx():
    return json.load(open(os.path.join(HERE, "golden", "reduce_fixtures.json")))


def test_dot_fixtures(fx):
    """vec.rs:1649-1673 dot_product and prod.rs:313-323 test_csvec_dot_by_binary_search: the same five numbers"""
    d = fx["dot"]
    for a, b, want in d["sparse"]:
        va, vb = d[a], d[b]
        assert ref.dot_merge(va["indices"], va["data"], vb["indices"], vb["data"]) == want
        assert ref.dot_by_binary_search(va["indices"], va["data"], vb["indices"], vb["data"]) == want
    assert ref.dot_dense(d["vec1"]["indices"], d["vec1"]["data"], d["dense"]) == d["vec1_dot_dense"]
    assert len(d["mismatch_dense"]) != d["dim"] and d["mismatch_sparse_dim"] != d["dim"]


def test_norm_fixtures(fx):
    """vec.rs:1691-1766"""
    n = fx["norms"]
    assert ref.squared_l2_norm([]) == 0.0 and ref.l2_norm([]) == 0.0 and ref.l1_norm([]) == 0.0
    v = n["vec"]
    assert ref.squared_l2_norm(v["data"]) == n["vec_squared_l2"] == ref.dot_merge(v["indices"], v["data"], v["indices"], v["data"])
    assert ref.l2_norm(v["data"]) == math.sqrt(n["vec_squared_l2"])
    assert ref.l1_norm(n["l1_vec"]["data"]) == n["l1"]
    for p, want in n["norm_empty"]:
        assert ref.norm([], float(p)) == want
    w = n["norm_vec"]["data"]
    assert ref.norm(w, math.inf) == n["norm_inf"] and ref.norm(w, -math.inf) == n["norm_neg_inf"] and ref.norm(w, 0.0) == n["norm_0"]
    assert abs(ref.l1_norm(w) - ref.norm(w, 1.0)) < n["norm_close"] and abs(ref.l2_norm(w) - ref.norm(w, 2.0)) < n["norm_close"]


def test_norm_quirks():
    """f64::max ignores NaN: a vector of NaNs only has norm(+inf) = -inf and norm(-inf) = +inf; NaN counts for p = 0"""
    nan = float("nan")
    assert ref.norm([nan, nan], math.inf) == -math.inf and ref.norm([nan], -math.inf) == math.inf
    assert ref.norm([nan, 3.0, -5.0], math.inf) == 5.0 and ref.norm([nan, 3.0, -5.0], -math.inf) == 3.0
    assert ref.norm([0.0, -0.0, nan, 2.0], 0.0) == 2.0
    assert ref.norm([0.0, 4.0], -1.0) == 0.0                    # pow(0, -1) = inf, pow(inf, -1) = 0


def test_unit_normalize_fixtures(fx):
    """vec.rs:1717-1739"""
    u = fx["unit_normalize"]
    assert ref.unit_normalize([]).size == 0
    assert np.array_equal(ref.bits(ref.unit_normalize(u["zeros"]["data"])), ref.bits(np.zeros(3)))
    nrm = math.sqrt(u["norm_squared"])
    assert np.array_equal(ref.bits(ref.unit_normalize(u["vec"]["data"])), ref.bits([x / nrm for x in u["vec"]["data"]]))
    assert abs(ref.l2_norm(ref.unit_normalize(u["vec"]["data"])) - 1.0) < 1e-5


def test_nnz_index_fixtures(fx):
    """vec.rs:1768-1782"""
    q = fx["vec_nnz_index"]
    for index, want in q["queries"]:
        assert ref.nnz_index(q["indices"], index) == want


def test_binary_search_dot_is_the_merge_dot():
    """both add the matched products by ascending index from +0.0: the same bits whichever side is longer"""
    rng = np.random.default_rng(11)
    for trial in range(60):
        dim = int(rng.integers(1, 400))
        na, nb = int(rng.integers(0, dim + 1)), int(rng.integers(0, dim + 1))
        ai, bi = np.sort(rng.choice(dim, na, replace=False)), np.sort(rng.choice(dim, nb, replace=False))
        ad = rng.standard_normal(na) * 10.0 ** rng.uniform(-10, 10, na)
        bd = rng.standard_normal(nb) * 10.0 ** rng.uniform(-10, 10, nb)
        m = ref.dot_merge(ai, ad, bi, bd)
        assert ref.bits(m) == ref.bits(ref.dot_by_binary_search(ai, ad, bi, bd))
        assert ref.bits(m) == ref.bits(ref.dot_merge(bi, bd, ai, ad)) == ref.bits(ref.dot_by_binary_search(bi, bd, ai, ad))


def test_rival_orders():
    """the rivals are what they say: equal to the chain where the arithmetic is exact, and themselves on a hand case"""
    ints = [float(k) for k in range(1, 200)]
    assert ref.chain(ints) == ref.reversed_chain(ints) == ref.pairwise_tree(ints) == ref.strided_sum(ints) == 199 * 100
    t = [1e16, 1.0, -1e16, 1.0]
    assert ref.chain(t) == 1.0 and ref.reversed_chain(t) == 0.0 and ref.pairwise_tree(t) == 0.0 + (1e16 + 1.0) + (-1e16 + 1.0)
    assert ref.strided_sum(t, lanes=2) == (1e16 - 1e16) + (1.0 + 1.0)


@pytest.mark.parametrize("n", [n for n in ref.SEAMS if n >= 65])
def test_order_inputs_tell_the_orders_apart(n):
    """the condition of the GPU order test, checked here for the committed seeds: on order_case(n) the reversed chain, a pairwise
    tree and the 64-way strided sum each miss the chain's bits, for every reduction of the test"""
    dim, idx, data, x = ref.order_case(n)
    assert len(idx) == n == len(set(idx.tolist())) and idx.max() < dim and np.all(np.diff(idx) > 0)
    assert np.log10(np.abs(data).max() / np.abs(data).min()) > 20 or n < 100
    for name, terms in ref.order_terms(n).items():
        assert ref.rivals_differ(terms), name
    assert sum(1 for j in range(n) if -data[j] in data[:j]) >= n // 4 - 1      # the cancelling pairs are there


def test_seams_follow_the_kernel_constants():
    """the sizes of the GPU tests are relative to the constants of csvec_reduce.hpp"""
    src = open(os.path.join(os.path.dirname(HERE), "sprs_amd", "csrc", "csvec_reduce.hpp")).read()
    assert "constexpr int RD_BLOCK = %d;" % ref.BLOCK in src and "constexpr int RD_UNROLL = %d;" % ref.UNROLL in src
    assert ref.SEAMS == [0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025]


def test_entry_points_check_arguments_without_a_device():
    from sprs_amd import _ffi
    lib = _ffi.lib
    out = C.c_double()
    h = C.c_void_p()
    assert lib.sprs_hip_csvec_dot_f64(None, None, C.byref(out), None) == _ffi.INVALID_ARG
    assert lib.sprs_hip_csvec_dot_dense_f64(None, None, 0, C.byref(out), None) == _ffi.INVALID_ARG
    assert lib.sprs_hip_csvec_norm_f64(None, _ffi.NORM_L1, 0.0, C.byref(out), None) == _ffi.INVALID_ARG
    assert lib.sprs_hip_csvec_unit_normalize_f64(None, C.byref(h), None) == _ffi.INVALID_ARG
    assert lib.sprs_hip_csvec_nnz_index(None, 0, None, None, None, None) == _ffi.INVALID_ARG
    assert (_ffi.NORM_SQUARED_L2, _ffi.NORM_L2, _ffi.NORM_L1, _ffi.NORM_P) == (0, 1, 2, 3)
