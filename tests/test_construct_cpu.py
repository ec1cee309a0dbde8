"""The Python restatement of the reference's construction functions (tests/construct_ref.py) against the reference's own
expectations (sprs/src/sparse/construct.rs:162-319, kronecker.rs:101-152), its numpy twins against the line-by-line ones, every
panic message of the reference's #[should_panic] tests, and the argument checks of the new entry points that need no device.
(A matrix handle cannot be made without a device: the dimension, storage and width checks run in tests/test_construct_gpu.py,
which tests/test_construct_emu_cpu.py also runs on the CPU.)"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import construct_ref as R
from conftest import ROOT
from helpers import ragged_csr

CSR, CSC = R.CSR, R.CSC


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(ROOT, "tests", "golden", "construct_fixtures.json")) as f:
        return json.load(f)


def fmat(d):
    return R.mat(d["storage"], d["shape"], d["indptr"], d["indices"], d["data"])


def from_triplets(shape, triplets, storage):
    """TriMat::to_csr / to_csc of distinct triplets"""
    key = (lambda t: (t[0], t[1])) if storage == CSR else (lambda t: (t[1], t[0]))
    ts = sorted(triplets, key=key)
    outer = shape[0] if storage == CSR else shape[1]
    indptr = [0] * (outer + 1)
    for t in ts:
        indptr[(t[0] if storage == CSR else t[1]) + 1] += 1
    return R.mat(storage, shape, np.cumsum(indptr), [t[1] if storage == CSR else t[0] for t in ts], [float(t[2]) for t in ts])


def entries(m):
    """{(row, col): value}"""
    out = {}
    for o, vec in enumerate(R.outer_iterator(m)):
        for i, v in vec:
            out[(o, i) if m[0] == CSR else (i, o)] = float(v)
    return out


TWINS = {"ref": (R.same_storage_fast_stack, R.vstack, R.hstack, R.bmat, R.kronecker_product),
         "vec": (R.same_storage_fast_stack_vec, R.vstack_vec, R.hstack_vec, R.bmat_vec, R.kronecker_product_vec)}


@pytest.mark.parametrize("twin", ["ref", "vec"])
def test_reference_expectations_stacking(fx, twin):
    fast, vstack, hstack, bmat, _ = TWINS[twin]
    a, b = fmat(fx["mat1"]), fmat(fx["mat2"])
    want = fmat(fx["mat1_vstack_mat2"])
    assert R.same_mat(fast([a, b]), want)                                            # same_storage_fast_stack_ok
    assert R.same_mat(vstack([a, b]), want)                                          # vstack_trivial
    assert R.same_mat(hstack([R.transpose(a), R.transpose(b)]), R.transpose(want))   # hstack_trivial
    assert R.same_mat(vstack([R.to_csc(a), b]), want)                                # vstack_with_conversion
    c = fx["bmat_simple"]
    e5, e4 = (R.eye(n) for n in c["eye"])
    assert R.same_mat(bmat([[e5, None], [None, e4]]), fmat(c["expected"]))
    for c in fx["bmat_complex"]:
        blocks = [[None if name is None else fmat(fx[name]) for name in row] for row in c["blocks"]]
        assert R.same_mat(bmat(blocks), fmat(c["expected"]))


@pytest.mark.parametrize("twin", ["ref", "vec"])
@pytest.mark.parametrize("sa,sb", [(CSR, CSR), (CSR, CSC), (CSC, CSC), (CSC, CSR)])
def test_reference_expectations_kronecker(fx, twin, sa, sb):
    c = fx["kronecker"]
    a, b = from_triplets(c["a"]["shape"], c["a"]["triplets"], sa), from_triplets(c["b"]["shape"], c["b"]["triplets"], sb)
    res = TWINS[twin][4](a, b)
    assert res[0] == sa and res[1] == (6, 6)
    assert entries(res) == {(r, col): float(v) for r, col, v in c["expected"]} and len(c["expected"]) == 16


def test_reference_panic_messages(fx):
    a, c, d = fmat(fx["mat1"]), fmat(fx["mat3"]), fmat(fx["mat4"])
    for fast, _, _, bmat, _ in TWINS.values():
        with pytest.raises(AssertionError, match="Empty stacking list"):             # same_storage_fast_stack_fail_empty_stacking_list
            fast([])
        with pytest.raises(AssertionError, match="Dimension mismatch"):              # ..._fail_dim_mismatch
            fast([a, c])
        with pytest.raises(AssertionError, match="Storage mismatch"):                # ..._fail_storage
            fast([a, d])
        with pytest.raises(AssertionError, match="Dimension mismatch"):              # bmat_fail_shapes
            bmat([[None, None], [None]])
        with pytest.raises(AssertionError, match="Empty stacking list"):             # bmat_fail_empty_stacking_list
            bmat([[]])
        with pytest.raises(AssertionError, match="Empty stacking list"):
            bmat([])
        with pytest.raises(AssertionError, match="Empty bmat row"):                  # bmat_fail_empty_bmat_row
            bmat([[None, None], [a, c]])
        with pytest.raises(AssertionError, match="Empty bmat col"):                  # bmat_fail_empty_bmat_col
            bmat([[c, None], [a, None]])
        with pytest.raises(AssertionError, match="Dimension mismatch"):              # hstack's inner-dimension check inside bmat
            bmat([[a, R.zero((4, 2))]])
        with pytest.raises(AssertionError, match="Dimension mismatch"):              # vstack's inside bmat
            bmat([[a], [c]])
    # the order of precedence: the list's shape before the dimensions, the dimensions before the storages
    with pytest.raises(AssertionError, match="Dimension mismatch"):
        R.same_storage_fast_stack([a, R.transpose(c)])


def _ragged(seed, rows, cols, storage, maxlen):
    """rows x cols in the given storage: ragged outer slices, a third of them empty"""
    rng = np.random.default_rng(seed)
    outer, inner = (rows, cols) if storage == CSR else (cols, rows)
    lens = rng.integers(0, maxlen + 1, size=outer)
    lens[rng.random(outer) < 0.3] = 0
    shape, ip, ix, dt = ragged_csr(np.minimum(lens, inner), inner, seed=seed, positive=False)
    m = R.mat(CSR, shape, ip, ix, dt)
    return m if storage == CSR else R.transpose(m)


@pytest.mark.parametrize("seed", range(4))
def test_numpy_twins_against_line_by_line(seed):
    a, b = _ragged(seed, 7, 9, CSR, 5), _ragged(seed + 10, 6, 9, CSR, 9)
    at, bt = R.to_other_storage(a), R.to_other_storage(b)
    assert R.same_mat(R.to_other_storage_vec(a), at) and R.same_mat(R.to_other_storage_vec(bt), R.to_owned(b))
    for x, y in ((a, b), (a, bt), (at, bt), (at, b)):
        assert R.same_mat(R.kronecker_product_vec(x, y), R.kronecker_product(x, y))
        assert R.same_mat(R.vstack_vec([x, y, x]), R.vstack([x, y, x]))
    h1, h2 = _ragged(seed + 20, 7, 4, CSC, 3), _ragged(seed + 30, 7, 0, CSR, 0)
    assert R.same_mat(R.hstack_vec([a, h1, h2]), R.hstack([a, h1, h2]))
    assert R.same_mat(R.same_storage_fast_stack_vec([at, h1, at]), R.same_storage_fast_stack([at, h1, at]))
    blocks = [[a, None, h1], [None, _ragged(seed + 40, 3, 2, CSC, 2), None]]
    assert R.same_mat(R.bmat_vec(blocks), R.bmat(blocks))
    # a slice view (indptr with a base) is read from its base
    view = (CSR, (3, 9), a[2][2:6], a[3][a[2][2]:], a[4][a[2][2]:])
    assert R.same_mat(R.kronecker_product_vec(view, b), R.kronecker_product(view, b))
    assert nnz_of(R.kronecker_product(view, b)) == R.nnz(view) * R.nnz(b)


def nnz_of(m):
    return int(m[2][-1])


def test_unaligned_bmat_of_the_reference():
    """the reference hstacks every super-row and vstacks the results: [2 | 3] over [3 | 2] columns is accepted, and a block's
    column offset is the sum of the ACTUAL widths to its left"""
    blk = lambda r, c, v: R.mat(CSR, (r, c), np.arange(r + 1), np.full(r, c - 1), np.full(r, float(v)))
    res = R.bmat([[blk(1, 2, 1), blk(1, 3, 2)], [blk(1, 3, 3), blk(1, 2, 4)]])
    assert res[1] == (2, 5) and res[3].tolist() == [1, 4, 2, 4] and res[4].tolist() == [1.0, 2.0, 3.0, 4.0]
    with pytest.raises(AssertionError, match="Dimension mismatch"):
        R.bmat([[blk(1, 2, 1), blk(1, 3, 2)], [blk(1, 3, 3), blk(1, 3, 4)]])


def test_argument_checks_need_no_device():
    from sprs_amd import _ffi
    lib = _ffi.lib
    h = C.c_void_p(0xDEAD)
    one = (C.c_void_p * 2)()                        # two NULL handles
    msg = lambda: lib.sprs_hip_last_error().decode()
    assert lib.sprs_hip_csmat_kronecker_f64(None, None, C.byref(h), None) == _ffi.INVALID_ARG and "NULL" in msg()
    for entry in (lib.sprs_hip_csmat_same_storage_fast_stack, lib.sprs_hip_csmat_vstack, lib.sprs_hip_csmat_hstack):
        assert entry(one, 0, C.byref(h), None) == _ffi.INVALID_ARG and msg() == "Empty stacking list"
        assert entry(None, 0, C.byref(h), None) == _ffi.INVALID_ARG and msg() == "Empty stacking list"
        assert entry(None, 2, C.byref(h), None) == _ffi.INVALID_ARG and "NULL" in msg()
        assert entry(one, 2, C.byref(h), None) == _ffi.INVALID_ARG and "NULL" in msg()
        assert entry(one, 0, None, None) == _ffi.INVALID_ARG and "NULL" in msg()
    assert lib.sprs_hip_csmat_bmat(one, 0, 2, C.byref(h), None) == _ffi.INVALID_ARG and msg() == "Empty stacking list"
    assert lib.sprs_hip_csmat_bmat(one, 2, 0, C.byref(h), None) == _ffi.INVALID_ARG and msg() == "Empty stacking list"
    assert lib.sprs_hip_csmat_bmat(None, 1, 2, C.byref(h), None) == _ffi.INVALID_ARG and "NULL" in msg()
    assert lib.sprs_hip_csmat_bmat(one, 1, 2, None, None) == _ffi.INVALID_ARG and "NULL" in msg()
    assert lib.sprs_hip_csmat_bmat(one, 1, 2, C.byref(h), None) == _ffi.INVALID_ARG and msg() == "Empty bmat row"
    assert h.value == 0xDEAD                        # *out is written on success only
    # the wrapper refuses the lists the C entry cannot express, with the reference's texts
    from sprs_amd import SprsHipError, construct
    for bad, text in (([], "Empty stacking list"), ([[]], "Empty stacking list"), ([[None, None], [None]], "Dimension mismatch")):
        with pytest.raises(SprsHipError) as e:
            construct.bmat(bad)
        assert str(e.value).endswith(text)
    with pytest.raises(SprsHipError) as e:
        construct.vstack([])
    assert e.value.status == _ffi.INVALID_ARG and str(e.value).endswith("Empty stacking list")
