"""The device triangular solves (tests/test_trisolve_gpu.py) past one chunk per wave: tri_solve_kernel launches one workgroup of
four waves per CU and a wave draws 64 positions of the level order at a time, so only with more than 256 x CUs rows does a wave
draw again.  Here: all four solves at that size, two singular rows in the first and in a late chunk, and a right-hand side that
holds the NaN whose bits are the "pending" tag of the work vector.  Every comparison is with the restatement tests/trisolve_ref.py,
bit for bit; where it yields NaNs, their positions and every other bit.

The matrix is full and non-symmetric (the other triangle is stored and must be ignored), strictly diagonally dominant, and made of
independent diagonal blocks of 97 rows — not a multiple of 64, so chunks straddle blocks — with short dependency chains: the
tests are about the redraw, not about hand-off latency.

The NaN case also runs against the kernel emulator (tests/test_trisolve_emu_cpu.py)."""
import numpy as np
import pytest

import trisolve_ref as ref
from test_trisolve_gpu import EMU, KINDS, arrays, device_mat, gpu_fn, gpu_solve, hip  # noqa: F401

pytestmark = pytest.mark.gpu

BLOCK = 97
ALL_ONES = np.frombuffer(np.uint64(0xFFFFFFFFFFFFFFFF).tobytes(), dtype=np.float64)[0]


def _cus():
    if EMU:
        return 4                                            # tests/emu/hip/hip_runtime.h
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def block_system(n, seed):
    """scipy CSR: inside every block of 97 rows the entries (r, r - 1), (r, r + 1), (r, r - 4) on every third row and (r, r + 4)
    on the others; all values differ, the diagonal is above the row's absolute sum"""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    r = np.arange(n)
    off = r % BLOCK
    size = np.minimum(BLOCK, n - (r - off))                  # (the last block is shorter)
    third = r % 3 == 0
    parts = [(r[off >= 1], r[off >= 1] - 1), (r[off + 1 < size], r[off + 1 < size] + 1),
             (r[third & (off >= 4)], r[third & (off >= 4)] - 4), (r[~third & (off + 4 < size)], r[~third & (off + 4 < size)] + 4)]
    rows, cols = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    a = sp.coo_matrix((rng.standard_normal(rows.size) * 3.0, (rows, cols)), shape=(n, n)).tocsr()
    a = (a + sp.diags(np.abs(a).sum(axis=1).A1 + 1.0 + rng.random(n))).tocsr()
    a.sort_indices()
    return a


def level_positions(kind, a):
    """position of every row in the order the solve walks: by level (the recurrence of trisolve_ref.levels), rows ascending
    inside a level"""
    n = a.shape[0]
    m = a.tocsr()
    ip, ix = m.indptr.tolist(), m.indices.tolist()
    upper = kind.startswith("u")
    lv = [0] * n
    for r in (range(n - 1, -1, -1) if upper else range(n)):
        for p in range(ip[r], ip[r + 1]):
            c = ix[p]
            if (c > r) if upper else (c < r):
                lv[r] = max(lv[r], lv[c] + 1)
    pos = np.empty(n, dtype=np.int64)
    pos[np.lexsort((np.arange(n), np.array(lv)))] = np.arange(n)
    return pos


_SHARED = {}


def redraw_system():
    """(n, matrix, b) at the redraw size, built once"""
    if "redraw" not in _SHARED:
        n = 256 * _cus() + 129
        _SHARED["redraw"] = (n, block_system(n, 256), np.random.default_rng(257).standard_normal(n) * 7.0 + 0.25)
    return _SHARED["redraw"]


def redraw_reference(kind):
    if kind not in _SHARED:
        n, a, b = redraw_system()
        ip, ix, dt = arrays(a, kind)
        _SHARED[kind] = (ref.SOLVES[kind](n, ip, ix, dt, b), ref.levels(kind, n, ip, ix))
    return _SHARED[kind]


# ---- 1. every wave draws a second chunk --------------------------------------------------------------------------------------------

@pytest.mark.skipif(EMU, reason="more than 256 x CUs rows of hand-offs: real device only")
@pytest.mark.parametrize("kind", KINDS)
def test_solve_redraws(hip, kind):
    n, a, b = redraw_system()
    assert n > 256 * _cus(), "the grid covers the system: no wave draws a second chunk"
    x_ref, levels = redraw_reference(kind)
    assert np.isfinite(x_ref).all()
    ip, ix, dt = arrays(a, kind)
    x, res = gpu_solve(kind, n, ip, ix, dt, b, np.uint32, np.uint64)
    assert np.array_equal(x, x_ref)
    assert res.levels == levels
    if kind.startswith("u"):                                 # one matrix, two walk directions: the bits must tell them apart
        assert not np.array_equal(redraw_reference("usolve_csr")[0], redraw_reference("usolve_csc")[0])


# ---- 2. the NaN whose bits are the work vector's "pending" tag ---------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_all_ones_nan_in_rhs(hip, kind):
    """b[100] is the NaN that memset 0xFF leaves: unknown 100 publishes it, and the unknowns that wait for it must see a value,
    not "pending" (the spin guard would end the call with an error)"""
    n, at = 200, 100
    a = block_system(n, 200)
    ip, ix, dt = arrays(a, kind)
    b = np.random.default_rng(201).standard_normal(n)
    b[at] = ALL_ONES
    assert b.view(np.uint64)[at] == 2**64 - 1
    x_ref = ref.SOLVES[kind](n, ip, ix, dt, b)
    nans = np.isnan(x_ref)
    assert nans[at] and 1 < nans.sum() < n                   # others depend on it; the other blocks stay finite
    x, res = gpu_solve(kind, n, ip, ix, dt, b)
    assert np.array_equal(np.isnan(x), nans)
    assert np.array_equal(x[~nans], x_ref[~nans])
    assert res.levels == ref.levels(kind, n, ip, ix)


# ---- 3. two singular rows: one in the first chunk, one in a chunk past 256 x CUs -------------------------------------------------------

def _without(a, missing, zeros):
    """the CSR and CSC arrays of `a` with the diagonal entries `missing` not stored and the diagonal entries `zeros` stored as 0.0"""
    c = a.tocoo()
    keep = ~((c.row == c.col) & np.isin(c.row, missing))
    data = np.where((c.row == c.col) & np.isin(c.row, zeros), 0.0, c.data)
    r, col, d = c.row[keep], c.col[keep], data[keep]
    n = a.shape[0]
    out = {}
    for name, outer, inner in (("csr", r, col), ("csc", col, r)):
        order = np.lexsort((inner, outer))
        ip = np.concatenate([[0], np.cumsum(np.bincount(outer, minlength=n))]).astype(np.uint64)
        out[name] = (ip, inner[order].astype(np.uint64), d[order])
    return out


@pytest.mark.skipif(EMU, reason="more than 256 x CUs rows of hand-offs: real device only")
@pytest.mark.parametrize("kind", KINDS)
def test_singular_rows_in_two_chunks(hip, kind):
    """test_singular_matrices of tests/test_trisolve_gpu.py where waves redraw: a diagonal that is not stored in the first chunk of
    the order, a stored 0.0 in a chunk that only a second draw reaches; the lower solves report the smaller index, the upper ones
    the larger"""
    from sprs_amd import _ffi
    from sprs_amd.device import DeviceVec
    n, a, b = redraw_system()
    grid_rows = 256 * _cus()
    assert n > grid_rows
    upper = kind.startswith("u")
    pos = level_positions(kind, a)
    # level 0 of a lower solve: the first row of every block; of an upper solve: the last.  The last level: the other end
    near = 5 * BLOCK + (BLOCK - 1 if upper else 0)
    far = (n // BLOCK - 3) * BLOCK + (0 if upper else BLOCK - 1)
    assert pos[near] < 64 and pos[far] >= grid_rows, "the two rows are not in the first chunk and in a redrawn one"
    missing, zeros = [near], [far]
    ip, ix, dt = _without(a, missing, zeros)["csc" if kind.endswith("csc") else "csr"]
    with pytest.raises(ref.Singular) as want:
        ref.SOLVES[kind](n, ip, ix, dt, b)
    assert want.value.index == (max if upper else min)(near, far)
    handle = device_mat(kind, n, ip, ix, dt)
    with pytest.raises(_ffi.SprsHipError) as e:
        gpu_fn(kind)(handle, DeviceVec.from_host(b))
    assert e.value.status == _ffi.SINGULAR_MATRIX
    assert e.value.index == want.value.index
    assert str(want.value) in str(e.value)
    structural = kind.endswith("csc") and want.value.index in missing
    assert e.value.reason == ("structural" if structural else "numeric")
    assert ("structural" in want.value.reason) == structural
