"""tests/structure_ref.py — the numpy restatement the device tests compare with — pinned on the reference's own constructor
tests (tests/golden/structure_fixtures.json, from sprs/src/sparse/csmat.rs:2345-2568).  No device."""
import json
import os

import numpy as np
import pytest

import structure_ref as R
from conftest import ROOT


def _fixtures():
    with open(os.path.join(ROOT, "tests", "golden", "structure_fixtures.json")) as f:
        return json.load(f)


FX = _fixtures()
IDS = [c["name"] for c in FX["matrices"]]


def _dims(c):
    rows, cols = c["shape"]
    return (cols, rows) if c["storage"] == R.CSR else (rows, cols)


@pytest.mark.parametrize("c", FX["matrices"], ids=IDS)
def test_check_compressed_structure_on_the_reference_cases(c):
    inner, outer = _dims(c)
    got = R.check_compressed_structure(inner, outer, np.array(c["indptr"], dtype=np.uint64), np.array(c["indices"], dtype=np.uint64))
    assert got == (c["check"]["kind"], c["check"]["text"], c["check"]["outer"])


# (new_from_unsorted has no indptr-length finding of its own — the reference panics on the slice — so that case is left to the check)
@pytest.mark.parametrize("c", [c for c in FX["matrices"] if c["name"] != "test_new_csr_bad_indptr_length"], ids=IDS[1:])
def test_new_from_unsorted_on_the_reference_cases(c):
    want = c["from_unsorted"]
    res, mat = R.new_from_unsorted(c["storage"], c["shape"], np.array(c["indptr"], dtype=np.uint64), np.array(c["indices"], dtype=np.uint64),
                                   np.array(c["data"]))
    assert res == (want["kind"], want["text"], want["outer"])
    if want["kind"] == R.OK:
        assert R.same_mat(mat, (c["shape"], c["indptr"], want["indices"], want["data"]))
    else:
        assert mat is None


def test_the_fixture_file_holds_every_recorded_case():
    assert len(IDS) == 10 and len(set(IDS)) == 10
    assert {"test_new_csr_fail_indices_ordering", "owned_csr_unsorted_indices", "new_csr_with_empty_row"} <= set(IDS)
    assert FX["vectors"] == []


def test_sorted_slices_are_skipped_and_values_travel_as_bits():
    """a sorted slice keeps its entries where they are; -0.0, 0.0, inf and a NaN payload arrive bit for bit"""
    dt = np.array([-0.0, 0.0, np.inf, 1.0, 2.0, 3.0])
    dt.view(np.uint64)[3] = 0x7FF8000000ABCDEF
    res, mat = R.new_from_unsorted(R.CSR, (2, 8), [0, 3, 6], [5, 1, 3, 0, 2, 7], dt)
    assert res == R.GOOD
    assert mat[2].tolist() == [1, 3, 5, 0, 2, 7]
    assert mat[3].view(np.uint64).tolist() == dt.view(np.uint64)[[1, 2, 0, 3, 4, 5]].tolist()


def test_precedence_of_the_findings():
    # the lowest offending slice wins, whichever kind it is
    assert R.check_compressed_structure(4, 2, [0, 2, 4], [0, 4, 1, 0])[::2] == (R.OUT_OF_RANGE, 0)
    assert R.check_compressed_structure(4, 2, [0, 2, 4], [1, 0, 0, 4])[::2] == (R.UNSORTED, 0)
    # inside one slice Unsorted wins; a duplicate next to an index >= inner is Unsorted after the sort too
    assert R.check_compressed_structure(4, 1, [0, 3], [1, 1, 9])[::2] == (R.UNSORTED, 0)
    assert R.new_from_unsorted(R.CSR, (1, 4), [0, 3], [9, 1, 1], [1., 2., 3.])[0][::2] == (R.UNSORTED, 0)
    assert R.new_from_unsorted(R.CSR, (1, 4), [0, 3], [9, 1, 2], [1., 2., 3.])[0][::2] == (R.OUT_OF_RANGE, 0)
    # a last index of inner - 1 passes, inner does not
    assert R.check_compressed_structure(4, 1, [0, 2], [0, 3]) == R.GOOD
    assert R.check_compressed_structure(4, 1, [0, 2], [0, 4])[0] == R.OUT_OF_RANGE
    # a negative value of a signed array is a large index
    assert R.check_compressed_structure(4, 1, [0, 2], np.array([0, -1], dtype=np.int64))[0] == R.OUT_OF_RANGE
    # the indptr: a decreasing pair, a total one above / below nnz, and the widths
    assert R.check_compressed_structure(4, 2, [0, 2, 1], [0])[1] == "Unsorted indptr"
    assert R.check_compressed_structure(4, 2, [0, 1, 3], [0, 1])[1] == "Indices length and inpdtr's nnz do not match"
    assert R.check_compressed_structure(4, 2, [0, 1, 1], [0, 1])[1] == "Indices length and inpdtr's nnz do not match"
    assert R.check_compressed_structure(1 << 32, 1, [0, 0], [], idx_bits=32)[1] == "Index type not large enough for this matrix"
    assert R.check_compressed_structure(4, (1 << 32) - 1, np.zeros(1 << 4), [], iptr_bits=32)[0] == R.SIZE_MISMATCH


def test_vectors_follow_try_new():
    assert R.check_vec(5, [0, 2, 4]) == R.GOOD
    assert R.check_vec(5, [0, 2, 5]) == (R.SIZE_MISMATCH, "indices larger than vector size", 0)
    assert R.check_vec(5, [2, 0]) == (R.UNSORTED, "Unsorted indices", 0)
    assert R.check_vec(1 << 32, [], idx_bits=32) == (R.OUT_OF_RANGE, "Index size is too small", 0)
    res, v = R.vec_new_from_unsorted(8, [7, 1, 4], [1., 2., 3.])
    assert res == R.GOOD and v[1].tolist() == [1, 4, 7] and v[2].tolist() == [2., 3., 1.]
    assert R.vec_new_from_unsorted(8, [7, 1, 7], [1., 2., 3.])[0] == (R.UNSORTED, "Unsorted indices", 0)
    assert R.vec_new_from_unsorted(8, [8, 1, 4], [1., 2., 3.])[0] == (R.SIZE_MISMATCH, "indices larger than vector size", 0)
    # a sorted vector with its last index out of range is not sorted again: the first check's finding stands
    assert R.vec_new_from_unsorted(8, [1, 9], [1., 2.])[0][0] == R.SIZE_MISMATCH
