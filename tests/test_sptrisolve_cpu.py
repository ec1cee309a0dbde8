"""CPU checks of the sparse-rhs triangular solve's yardstick and boundary: the plain-Python restatement
(tests/sptrisolve_ref.py) reproduces the reference's own test systems, its two orders agree bit for bit wherever the
arithmetic is exact, and the C entry point is there and refuses NULL arguments without a device."""
import ctypes as C
import json
import os
from fractions import Fraction

import numpy as np

import sptrisolve_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))


def fixtures():
    return json.load(open(os.path.join(HERE, "golden", "sptrisolve_fixtures.json")))["systems"]


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def test_restatement_reproduces_the_fixtures():
    """trisolve.rs:445-517: the pattern and its values as a set, from a workspace that the reference fills with ones"""
    systems = fixtures()
    assert len(systems) == 2
    for s in systems:
        n = s["shape"][0]
        want = dict(zip(s["x_indices"], [float(v) for v in s["x_data"]]))
        for solve in (ref.reference_order, ref.ascending):
            pat, val = solve(n, s["indptr"], s["indices"], s["data"], s["rhs_indices"], s["rhs_data"])
            assert dict(zip(pat, val.tolist())) == want and len(pat) == len(want)
        pat, _ = ref.ascending(n, s["indptr"], s["indices"], s["data"], s["rhs_indices"], s["rhs_data"])
        assert pat == sorted(pat) == ref.reach(n, s["indptr"], s["indices"], s["rhs_indices"])


def _exact_solution(n, ip, ix, dt, ri, rv):
    """the solution over the rationals, by ascending column"""
    x = [Fraction(0)] * n
    for i, v in zip(ri, rv):
        x[int(i)] = Fraction(float(v))
    pat = ref.reach(n, ip, ix, ri)
    for c in pat:
        col = {int(ix[p]): Fraction(float(dt[p])) for p in range(int(ip[c]), int(ip[c + 1]))}
        x[c] = x[c] / col[c]
        for r, v in col.items():
            if r > c:
                x[r] -= v * x[c]
    return [x[c] for c in pat]


def test_the_two_orders_agree_bit_for_bit_on_exact_systems():
    """dyadic values, power-of-two diagonals, small integer right-hand sides: every product, subtraction and division is exact
    (checked against the rationals), so the order of the columns cannot show"""
    fill_in = 0
    for seed in range(20):
        n = 200
        ip, ix, dt = ref.exact_system(n, seed)
        rng = np.random.default_rng(1000 + seed)
        ri = np.sort(rng.choice(n, int(rng.integers(1, 12)), replace=False))
        rv = rng.integers(-8, 9, ri.size).astype(np.float64)            # (zeros among them: roots all the same)
        p_ref, v_ref = ref.reference_order(n, ip, ix, dt, ri, rv)
        p_asc, v_asc = ref.ascending(n, ip, ix, dt, ri, rv)
        assert sorted(p_ref) == p_asc and len(set(p_ref)) == len(p_ref)
        exact = _exact_solution(n, ip, ix, dt, ri, rv)
        assert all(Fraction(float(v)) == e for v, e in zip(v_asc, exact)), "the generator left the exact range"
        by_index = dict(zip(p_ref, _bits(v_ref).tolist()))
        assert [by_index[c] for c in p_asc] == _bits(v_asc).tolist()
        fill_in += len(p_asc) - ri.size
    assert fill_in > 100                                                # the systems do produce fill-in


def test_reference_order_is_not_sorted_and_ascending_is():
    """the contract difference (a): the right stack is a topological order, not an ascending one"""
    ip, ix, dt = ref.csc_arrays(4, [0, 1, 2, 3, 3, 2], [0, 1, 2, 3, 0, 1], [1.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    p_ref, _ = ref.reference_order(4, ip, ix, dt, [0, 1], [1.0, 1.0])
    p_asc, _ = ref.ascending(4, ip, ix, dt, [0, 1], [1.0, 1.0])
    assert p_asc == [0, 1, 2, 3] and sorted(p_ref) == p_asc and p_ref != p_asc


def test_symbol_signature_and_null_arguments():
    from sprs_amd import _ffi, linalg
    assert "sprs_hip_lsolve_csc_sparse_rhs_f64" in _ffi.SIGNATURES and hasattr(linalg, "lsolve_csc_sparse_rhs")
    fn = _ffi.lib.sprs_hip_lsolve_csc_sparse_rhs_f64
    assert fn(None, None, None, None, None) == _ffi.INVALID_ARG
    out = C.c_void_p(1)
    assert fn(None, None, C.byref(out), None, None) == _ffi.INVALID_ARG and not out.value      # *out is NULL after a failure
    assert b"NULL" in _ffi.lib.sprs_hip_last_error()
    info = linalg._SpTriInfo()
    assert C.sizeof(info) == 48 and linalg._SpTriInfo.singular_reason.offset == 40
    import sprs_amd
    assert sprs_amd.get_option("sptrisolve_budget") == 4096
