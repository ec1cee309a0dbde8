"""GPU parity tests of the device sparse-rhs lower triangular solve (twin of lsolve_csc_sparse_rhs,
sprs/src/sparse/linalg/trisolve.rs:286-358) against the plain-Python restatement of tests/sptrisolve_ref.py: the pattern
index for index (the reach, ascending) and every value bit for bit against `ascending`; on exact-arithmetic inputs also
against the reference's own depth-first order.  (tests/test_sptrisolve_emu_cpu.py runs this file through the CPU emulator of
the kernels as well.)"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import sptrisolve_ref as ref
import trisolve_ref

pytestmark = pytest.mark.gpu

EMU = "emu" in os.path.basename(os.environ.get("SPRS_HIP_LIBRARY", ""))
NARROW_VERTICES, NARROW_ENTRIES = 1024, 4096          # the narrow kernel's caps (sptrisolve.hpp)


@pytest.fixture(scope="module")
def hip():
    import sprs_amd
    if sprs_amd.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X (no CPU fallback exists)")
    return sprs_amd


def device_mat(n, ip, ix, dt, idx=np.uint64, ptr=np.uint64):
    from sprs_amd.device import DeviceCsMat, CSC
    return DeviceCsMat.from_host((n, n), ip.astype(ptr), ix.astype(idx), dt, storage=CSC)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def solve(mat, n, ri, rv, vidx=np.uint64):
    from sprs_amd.device import DeviceCsVec
    from sprs_amd.linalg import lsolve_csc_sparse_rhs
    return lsolve_csc_sparse_rhs(mat, DeviceCsVec.from_host(n, np.asarray(ri).astype(vidx), np.asarray(rv, dtype=np.float64)))


def check(n, ip, ix, dt, ri, rv, mat=None, idx=np.uint64, ptr=np.uint64, vidx=np.uint64, exact=False):
    """one solve against `ascending` (and, with exact, against the reference's own order); returns the device result"""
    ri, rv = np.asarray(ri, dtype=np.int64), np.asarray(rv, dtype=np.float64)
    pat, val = ref.ascending(n, ip, ix, dt, ri, rv)
    out = solve(mat if mat is not None else device_mat(n, ip, ix, dt, idx, ptr), n, ri, rv, vidx)
    dim, oi, ov = out.to_host()
    assert dim == n and oi.dtype.itemsize == np.dtype(idx).itemsize
    assert oi.tolist() == pat
    assert np.array_equal(bits(ov), bits(val))
    assert out.reach == len(pat) and out.reach_levels == ref.depth(n, ip, ix, ri)
    if exact:
        p_ref, v_ref = ref.reference_order(n, ip, ix, dt, ri, rv)
        by_index = dict(zip(p_ref, bits(v_ref).tolist()))
        assert sorted(p_ref) == pat and [by_index[c] for c in pat] == bits(ov).tolist()
    return out, oi, ov


def random_lower(n, seed, per_col=3, span=None):
    """a lower triangular matrix with random real values: every column has its diagonal and up to per_col entries below it
    (at most `span` rows away)"""
    rng = np.random.default_rng(seed)
    rows, cols = list(range(n)), list(range(n))
    vals = list(rng.uniform(1.0, 2.0, n) * rng.choice([-1.0, 1.0], n))
    for c in range(n - 1):
        hi = n if span is None else min(n, c + 1 + span)
        for r in np.unique(rng.integers(c + 1, hi, per_col)):
            rows.append(int(r))
            cols.append(c)
            vals.append(float(rng.uniform(-1.0, 1.0)))
    return ref.csc_arrays(n, rows, cols, vals)


def banded_lower(n, offsets, seed):
    """diagonal plus the sub-diagonals `offsets`: the reach of index s is every index >= s when 1 is among them"""
    rng = np.random.default_rng(seed)
    rows, cols = list(range(n)), list(range(n))
    vals = list(rng.uniform(1.0, 2.0, n))
    for off in offsets:
        for c in range(n - off):
            rows.append(c + off)
            cols.append(c)
            vals.append(float(rng.uniform(-1.0, 1.0)))
    return ref.csc_arrays(n, rows, cols, vals)


# ---- the reference's own systems, random systems ----------------------------------------------------------------------------------

def test_golden_systems(hip):
    """trisolve.rs:445-517"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sptrisolve_fixtures.json")
    systems = json.load(open(path))["systems"]
    assert len(systems) == 2
    for s in systems:
        n = s["shape"][0]
        ip, ix = np.array(s["indptr"], dtype=np.uint64), np.array(s["indices"], dtype=np.uint64)
        _, oi, ov = check(n, ip, ix, np.array(s["data"], dtype=np.float64), s["rhs_indices"], s["rhs_data"], exact=True)
        assert oi.tolist() == s["x_indices"] and ov.tolist() == [float(v) for v in s["x_data"]]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_real_values(hip, seed):
    n = 257
    ip, ix, dt = random_lower(n, seed)
    rng = np.random.default_rng(50 + seed)
    ri = np.sort(rng.choice(n, 5, replace=False))
    out, oi, _ = check(n, ip, ix, dt, ri, rng.standard_normal(ri.size))
    assert ri.size < oi.size                                               # fill-in


@pytest.mark.parametrize("seed", [0, 7])
def test_exact_values_match_the_reference_order_too(hip, seed):
    n = 257
    ip, ix, dt = ref.exact_system(n, seed)
    rng = np.random.default_rng(seed)
    ri = np.sort(rng.choice(n, 9, replace=False))
    check(n, ip, ix, dt, ri, rng.integers(-8, 9, ri.size), exact=True)


# ---- bitmap and chunk seams ---------------------------------------------------------------------------------------------------------

def test_bitmap_word_seams_and_a_doubly_reached_vertex(hip):
    """indices on both sides of the 32-bit words of the bitmap and at n - 1; 64 is reachable from 31 and from 32 (one level:
    both are roots) and appears once"""
    n = 257
    rows = list(range(n)) + [64, 64, n - 1, 33]
    cols = list(range(n)) + [31, 32, 63, 31]
    vals = [2.0] * n + [1.0, 3.0, -1.0, 5.0]
    ip, ix, dt = ref.csc_arrays(n, rows, cols, vals)
    _, oi, _ = check(n, ip, ix, dt, [31, 32, 63], [1.0, 2.0, 3.0], exact=True)
    assert oi.tolist() == [31, 32, 33, 63, 64, n - 1]
    _, oi, _ = check(n, ip, ix, dt, [n - 1], [4.0], exact=True)
    assert oi.tolist() == [n - 1]


@pytest.mark.parametrize("reach", [65, 257, 1000])
def test_reach_spans_waves_workgroups_and_chunks(hip, reach):
    """every index from n - reach on: more than one wave (65), more than one workgroup (257), several chunks per wave (1000);
    rows receive up to three products"""
    n = 1100
    ip, ix, dt = banded_lower(n, (1, 7, 64), reach)
    out, oi, _ = check(n, ip, ix, dt, [n - reach], [1.5])
    assert oi.tolist() == list(range(n - reach, n))


# ---- what the pattern holds ---------------------------------------------------------------------------------------------------------

def test_fill_in_stored_zero_root_and_cancellation(hip):
    n = 6
    # | 1           |
    # | 1  1        |
    # |    2  1     |
    # |          4  |      column 3 is reached from nothing but itself
    # |          1 1|
    rows = [0, 1, 1, 2, 2, 3, 4, 4, 5]
    cols = [0, 0, 1, 1, 2, 3, 3, 4, 5]
    vals = [1.0, 1.0, 1.0, 2.0, 1.0, 4.0, 1.0, 1.0, 1.0]
    ip, ix, dt = ref.csc_arrays(n, rows, cols, vals)
    # fill-in: 2 is not stored in rhs; cancellation: x1 = 3 - 1 * 3 = 0 is kept, and so is x2 = 0 - 2 * 0
    _, oi, ov = check(n, ip, ix, dt, [0, 1], [3.0, 3.0], exact=True)
    assert oi.tolist() == [0, 1, 2] and ov[0] == 3.0 and ov[1] == 0.0 and ov[2] == 0.0
    # a stored 0.0 is a root: its column and what it reaches are in the pattern
    _, oi, ov = check(n, ip, ix, dt, [3], [0.0], exact=True)
    assert oi.tolist() == [3, 4] and not ov.any()


def test_full_reach_equals_the_dense_solve(hip):
    from sprs_amd.device import DeviceVec
    from sprs_amd.linalg import lsolve_csc_dense_rhs
    n = 257
    ip, ix, dt = random_lower(n, 11, per_col=4)
    b = np.random.default_rng(12).standard_normal(n)
    mat = device_mat(n, ip, ix, dt)
    _, oi, ov = check(n, ip, ix, dt, np.arange(n), b, mat=mat)
    x = DeviceVec.from_host(b)
    lsolve_csc_dense_rhs(mat, x)
    assert oi.tolist() == list(range(n)) and np.array_equal(bits(ov), bits(x.to_host()))
    assert np.array_equal(bits(ov), bits(trisolve_ref.lsolve_csc_dense_rhs(n, ip, ix, dt, b)))


def test_inf_and_nan_under_columns_outside_the_reach(hip):
    """(5, 3) = inf and (5, 4) = NaN: row 5 is in the reach, columns 3 and 4 are not; 0.0 * inf would be a NaN"""
    n = 10
    rows = list(range(n)) + [5, 5, 5, 7]
    cols = list(range(n)) + [0, 3, 4, 5]
    vals = [2.0] * n + [1.0, np.inf, np.nan, 4.0]
    ip, ix, dt = ref.csc_arrays(n, rows, cols, vals)
    _, oi, ov = check(n, ip, ix, dt, [0], [8.0], exact=True)
    assert oi.tolist() == [0, 5, 7] and ov.tolist() == [4.0, -2.0, 4.0]


def test_entries_above_the_diagonal(hip):
    """(2, 5) lies above the diagonal: the search follows it (2 and what column 2 reaches are in the pattern), the
    arithmetic skips it (row 2 receives nothing from column 5)"""
    n = 9
    rows = list(range(n)) + [5, 2, 6, 8]
    cols = list(range(n)) + [1, 5, 2, 5]
    vals = [2.0] * n + [1.0, 100.0, 3.0, -1.0]
    ip, ix, dt = ref.csc_arrays(n, rows, cols, vals)
    _, oi, ov = check(n, ip, ix, dt, [1], [4.0])
    assert oi.tolist() == [1, 2, 5, 6, 8] and ov.tolist() == [2.0, 0.0, -1.0, 0.0, -0.5]


# ---- singular columns -----------------------------------------------------------------------------------------------------------------

def _chain_with(n, missing=(), zeros=(), zero=0.0):
    """bidiagonal chain whose diagonal entries `missing` are not stored and whose diagonal entries `zeros` are stored `zero`"""
    rows = [i for i in range(n) if i not in missing] + list(range(1, n))
    cols = [i for i in range(n) if i not in missing] + list(range(n - 1))
    vals = [zero if i in zeros else 2.0 for i in range(n) if i not in missing] + [1.0] * (n - 1)
    return ref.csc_arrays(n, rows, cols, vals)


@pytest.mark.parametrize("missing,zeros,zero,index,reason", [
    ((70,), (), 0.0, 70, "structural"), ((), (70,), -0.0, 70, "numeric"), ((90,), (75,), 0.0, 75, "numeric"),
    ((75,), (90,), 0.0, 75, "structural")])
def test_singular_in_the_reach(hip, missing, zeros, zero, index, reason):
    from sprs_amd import _ffi
    n = 100
    ip, ix, dt = _chain_with(n, missing, zeros, zero)
    with pytest.raises(trisolve_ref.Singular) as want:
        ref.ascending(n, ip, ix, dt, [60], [1.0])
    assert want.value.index == index and reason in want.value.reason
    with pytest.raises(_ffi.SprsHipError) as e:
        solve(device_mat(n, ip, ix, dt), n, [60], [1.0])
    assert e.value.status == _ffi.SINGULAR_MATRIX and e.value.index == index and e.value.reason == reason
    assert str(want.value) in str(e.value)                                  # "Singular matrix at index {} ({reason})"


def test_singular_outside_the_reach_is_not_an_error(hip):
    from sprs_amd import _ffi
    from sprs_amd.device import DeviceVec
    from sprs_amd.linalg import lsolve_csc_dense_rhs
    n = 100
    ip, ix, dt = _chain_with(n, missing=(10,), zeros=(20,))
    mat = device_mat(n, ip, ix, dt)
    _, oi, _ = check(n, ip, ix, dt, [60], [1.0], mat=mat, exact=True)
    assert oi.tolist() == list(range(60, n))
    with pytest.raises(_ffi.SprsHipError) as e:
        lsolve_csc_dense_rhs(mat, DeviceVec.from_host(np.ones(n)))
    assert e.value.status == _ffi.SINGULAR_MATRIX and e.value.index == 10


# ---- depth ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("budget", [None, 7])
def test_chain_longer_than_the_step_budget(hip, budget):
    """a bidiagonal chain: one vertex per level; the narrow kernel hands back every `budget` levels and not once per level"""
    default = hip.get_option("sptrisolve_budget")
    if budget is None:
        budget = 24 if EMU else default                                     # (the emulator runs a level in milliseconds)
    hip.set_option("sptrisolve_budget", budget)
    try:
        depth = 2 * budget + 5
        n = depth + 3
        ip, ix, dt = banded_lower(n, (1,), 5)
        out, oi, _ = check(n, ip, ix, dt, [3], [1.0])
        assert oi.size == depth and out.reach_levels == depth
        assert out.reach_launches == -(-depth // budget) == 3
        hip.set_option("sptrisolve_budget", depth)                          # exactly one launch's worth: no launch to find the end
        out = solve(device_mat(n, ip, ix, dt), n, [3], [1.0])
        assert out.reach_launches == 1 and out.reach_levels == depth
    finally:
        hip.set_option("sptrisolve_budget", default)


def test_narrow_levels_near_their_caps(hip):
    """a frontier of 899 vertices with 2 697 stored entries stays in the one-workgroup kernel (at most 1024 and 4096): every
    lane expands several batches of entries, many of them leading to the same few rows, each claimed once"""
    fan, n = 900, 1500
    rows = list(range(n)) + list(range(1, fan))
    cols = list(range(n)) + [0] * (fan - 1)
    for c in range(1, fan):
        rows += [fan + (c * 7) % 500, fan + 500 + (c * 13) % 100]
        cols += [c, c]
    rng = np.random.default_rng(8)
    vals = list(rng.uniform(1.0, 2.0, n)) + list(rng.uniform(-1.0, 1.0, len(rows) - n))
    ip, ix, dt = ref.csc_arrays(n, rows, cols, vals)
    assert int(ip[fan] - ip[1]) == 3 * (fan - 1) <= NARROW_ENTRIES and fan - 1 <= NARROW_VERTICES
    out, oi, _ = check(n, ip, ix, dt, [0], [1.0])
    assert out.reach_levels == 3 and out.reach_launches == 1 and oi.size > fan + 400


def test_hub_column_then_a_chain(hip):
    """column 0 has more entries than the narrow kernel takes: narrow -> wide (the hub's entries) -> wide (its 5 000 rows) ->
    narrow again for the chain behind the last of them"""
    hub, tail = NARROW_ENTRIES + 904, 40
    n = hub + tail
    rows = list(range(n)) + list(range(1, hub)) + list(range(hub, n))
    cols = list(range(n)) + [0] * (hub - 1) + list(range(hub - 1, n - 1))
    rng = np.random.default_rng(3)
    vals = list(rng.uniform(1.0, 2.0, n)) + list(rng.uniform(-1.0, 1.0, hub - 1 + tail))
    ip, ix, dt = ref.csc_arrays(n, rows, cols, vals)
    assert ip[1] - ip[0] == hub > NARROW_ENTRIES and hub - 1 > NARROW_VERTICES
    out, oi, _ = check(n, ip, ix, dt, [0], [1.0])
    assert oi.size == n and out.reach_levels == 2 + tail
    assert out.reach_launches == 4


# ---- index widths, views, arguments -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("idx,ptr,vidx", [(np.uint16, np.uint16, np.uint64), (np.uint32, np.uint64, np.uint16), (np.uint64, np.uint32, np.uint32),
                                          (np.uint32, np.uint32, np.uint32)])
def test_index_widths(hip, idx, ptr, vidx):
    n = 130
    ip, ix, dt = random_lower(n, 21, span=20)
    check(n, ip, ix, dt, [3, 64], [1.0, -2.0], idx=idx, ptr=ptr, vidx=vidx)


def test_transpose_view_of_a_csr_matrix(hip):
    """the CSC arrays of L are the CSR arrays of its transpose: the view of that CSR handle is a CSC handle of L"""
    from sprs_amd.device import DeviceCsMat
    n = 90
    ip, ix, dt = random_lower(n, 31)
    upper = DeviceCsMat.from_host((n, n), ip, ix, dt)                       # CSR: L^T
    view = upper.transpose_view()
    assert view.is_csc()
    check(n, ip, ix, dt, [5, 40], [1.0, 2.0], mat=view)


def test_contract_violations(hip):
    from sprs_amd import _ffi
    from sprs_amd.device import DeviceCsMat, DeviceCsVec
    fn = _ffi.lib.sprs_hip_lsolve_csc_sparse_rhs_f64
    eye = DeviceCsMat.eye(4).to_other_storage()
    assert eye.is_csc()
    v4 = DeviceCsVec.from_host(4, np.array([1], dtype=np.uint64), np.ones(1))
    out = C.c_void_p()
    assert fn(eye._h, v4._h, None, None, None) == _ffi.INVALID_ARG
    assert fn(None, v4._h, C.byref(out), None, None) == _ffi.INVALID_ARG and fn(eye._h, None, C.byref(out), None, None) == _ffi.INVALID_ARG
    with pytest.raises(_ffi.SprsHipError) as e:                             # assert!(lower_tri_mat.is_csc(), "Storage mismatch")
        solve(DeviceCsMat.eye(4), 4, [1], [1.0])
    assert e.value.status == _ffi.INVALID_ARG and "Storage mismatch" in str(e.value)
    rect = DeviceCsMat.from_host((3, 2), np.array([0, 1, 2], dtype=np.uint64), np.array([0, 1], dtype=np.uint64), np.ones(2), storage=_ffi.CSC)
    with pytest.raises(_ffi.SprsHipError) as e:
        solve(rect, 3, [1], [1.0])
    assert e.value.status == _ffi.DIM_MISMATCH
    with pytest.raises(_ffi.SprsHipError) as e:
        solve(eye, 5, [1], [1.0])
    assert e.value.status == _ffi.DIM_MISMATCH and "Dimension mismatch" in str(e.value)
    # nothing stored in rhs, and n == 0: an empty vector
    res = solve(eye, 4, [], [])
    assert res.to_host()[0] == 4 and res.nnz() == 0 and res.reach == 0
    empty = DeviceCsMat.from_host((0, 0), np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint64), np.zeros(0), storage=_ffi.CSC)
    res = solve(empty, 0, [], [])
    assert res.dim() == 0 and res.nnz() == 0


def test_dimension_that_does_not_fit_the_declared_index_width(hip):
    """u16 indices hold every index of a 65 536-row matrix, but not the dimension of the result (I::from(n), vec.rs:446-451)"""
    from sprs_amd import _ffi
    from sprs_amd.device import DeviceCsMat
    n = 65536
    mat = DeviceCsMat.from_host((n, n), np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint16), np.ones(n), storage=_ffi.CSC)
    with pytest.raises(_ffi.SprsHipError) as e:
        solve(mat, n, [5], [1.0])
    assert e.value.status == _ffi.INDEX_OVERFLOW


# ---- the per-handle scratch -------------------------------------------------------------------------------------------------------------

def test_scratch_is_clean_between_solves_and_after_a_failure(hip):
    """one handle: a large reach, then a small one that must not see it; a singular failure (the scratch stays dirty), then
    a solve that must not see that either"""
    from sprs_amd import _ffi
    n = 400
    ip, ix, dt = _chain_with(n, zeros=(300,))
    # 310 -> 350 and 350 -> 399 beside the chain: rows 350 and 399 receive two products
    rows = np.concatenate([ix.astype(np.int64), [350, 399]])
    cols = np.concatenate([np.repeat(np.arange(n), np.diff(ip.astype(np.int64))), [310, 350]])
    ip, ix, dt = ref.csc_arrays(n, rows, cols, np.concatenate([dt, [0.5, 0.25]]))
    mat = device_mat(n, ip, ix, dt)
    big, _, _ = check(n, ip, ix, dt, [301, 305], [1.0, 2.0], mat=mat)
    assert big.reach == 99
    small, oi, _ = check(n, ip, ix, dt, [390], [3.0], mat=mat)
    assert oi.tolist() == list(range(390, n))
    with pytest.raises(_ffi.SprsHipError) as e:
        solve(mat, n, [10], [1.0])                                          # reaches the stored zero at 300
    assert e.value.status == _ffi.SINGULAR_MATRIX and e.value.index == 300
    check(n, ip, ix, dt, [395], [1.0], mat=mat)
    check(n, ip, ix, dt, [301, 350], [1.0, -1.0], mat=mat)
