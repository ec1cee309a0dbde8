"""Device check_compressed_structure and new_from_unsorted (sprs/src/sparse.rs:300-358, csmat.rs:311-401, vec.rs:536-557) against
tests/structure_ref.py — kind, text and first offending slice of every finding; indptr, indices and the uint64 view of the values
of every result, bit for bit, no tolerance anywhere.

The cases also run against the kernel emulator (tests/test_structure_emu_cpu.py), whose device blocks end at a guard page; the
torch cases need a real device."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import structure_ref as R
from conftest import IDX_COMBOS, ROOT

pytestmark = pytest.mark.gpu

EMULATED = bool(os.environ.get("SPRS_HIP_LIBRARY"))
CSR, CSC = R.CSR, R.CSC
NAN_PAYLOAD = 0x7FF8000000ABCDEF
TILE = 2048                                   # option perm_tile: entries per workgroup of the check
SEAM_LENGTHS = [0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 9000]
SEAM_INNER = 1 << 14


@pytest.fixture(scope="module", autouse=True)
def _need_device():
    import sprs_amd
    if sprs_amd.device_count() < 1:
        pytest.skip("no HIP device")


def _dev(arr, spare=0):
    """a raw device block holding arr (and `spare` more bytes)"""
    from sprs_amd import _ffi
    from sprs_amd.device import DeviceVec
    arr = np.ascontiguousarray(arr)
    block = DeviceVec((arr.nbytes + spare + 7) // 8 + 1)
    if arr.nbytes:
        _ffi.check(_ffi.lib.sprs_hip_memcpy_h2d(C.c_void_p(block.ptr), C.c_void_p(arr.ctypes.data), arr.nbytes))
    return block


def _wrap(shape, ip, ix, dt, storage=CSR, idx=np.uint64, ptr=np.uint64, nnz=None, spare=0):
    """sprs_hip_csmat_wrap_device over three raw device arrays: nothing is looked at on the way in"""
    from sprs_amd import _ffi
    from sprs_amd.device import DeviceCsMat
    ip, ix, dt = np.asarray(ip).astype(ptr), np.asarray(ix).astype(idx), np.asarray(dt, dtype=np.float64)
    keep = (_dev(ip), _dev(ix, spare * ix.itemsize), _dev(dt, spare * 8))
    h = C.c_void_p()
    _ffi.check(_ffi.lib.sprs_hip_csmat_wrap_device(C.byref(h), storage, shape[0], shape[1], ix.size if nnz is None else nnz, C.c_void_p(keep[0].ptr),
                                                   ip.itemsize, C.c_void_p(keep[1].ptr), ix.itemsize, C.c_void_p(keep[2].ptr)))
    return DeviceCsMat(h.value, keep=keep)


def _wrap_vec(dim, ix, dt, idx=np.uint64):
    from sprs_amd import _ffi
    from sprs_amd.device import DeviceCsVec
    ix, dt = np.asarray(ix).astype(idx), np.asarray(dt, dtype=np.float64)
    keep = (_dev(ix), _dev(dt))
    h = C.c_void_p()
    _ffi.check(_ffi.lib.sprs_hip_csvec_wrap_device(C.byref(h), dim, ix.size, C.c_void_p(keep[0].ptr), ix.itemsize, C.c_void_p(keep[1].ptr)))
    return DeviceCsVec(h.value, keep=keep)


def _finding(call):
    """(kind, text, outer) of the SprsHipError `call` raises, R.GOOD when it returns"""
    from sprs_amd import SprsHipError, _ffi
    try:
        call()
    except SprsHipError as e:
        assert e.status == _ffi.BAD_STRUCTURE
        return (e.kind, str(e).split(": ", 1)[1], e.outer)
    return R.GOOD


def _dims(shape, storage):
    return (shape[1], shape[0]) if storage == CSR else (shape[0], shape[1])


def _both(shape, ip, ix, dt, storage=CSR, idx=np.uint64, ptr=np.uint64, **kw):
    """check_structure and sort_indices of the wrapped arrays against the restatement; -> the sorted handle or None"""
    inner, outer = _dims(shape, storage)
    ip, ix = np.asarray(ip).astype(ptr), np.asarray(ix).astype(idx)
    m = _wrap(shape, ip, ix, dt, storage, idx, ptr, **kw)
    nnz = kw.get("nnz", ix.size)
    assert _finding(m.check_structure) == R.check_compressed_structure(inner, outer, ip, ix[:nnz])
    want, mat = R.new_from_unsorted(storage, shape, ip, ix[:nnz], np.asarray(dt, dtype=np.float64)[:nnz])
    got = []
    assert _finding(lambda: got.append(m.sort_indices())) == want
    if want[0] != R.OK:
        assert not got
        return None
    res = got[0]
    assert res.storage() == storage and res.index_bytes() == np.dtype(idx).itemsize and res.indptr_bytes() == np.dtype(ptr).itemsize
    assert R.same_mat(res.to_host(), mat)
    assert _finding(res.check_structure) == R.GOOD
    return res


def _special(n, seed):
    """random values with -0.0, explicit 0.0, inf and a NaN with a payload among them"""
    rng = np.random.default_rng(seed)
    dt = rng.standard_normal(n)
    dt[rng.random(n) < 0.04] = -0.0
    dt[rng.random(n) < 0.04] = 0.0
    dt[rng.random(n) < 0.02] = np.inf
    dt.view(np.uint64)[rng.random(n) < 0.02] = NAN_PAYLOAD
    if n >= 4:
        dt[:3] = [-0.0, 0.0, np.inf]
        dt.view(np.uint64)[3] = NAN_PAYLOAD
    return dt


# ---- 1. the reference's own constructor tests (csmat.rs:2345-2568) ------------------------------------------------------------

with open(os.path.join(ROOT, "tests", "golden", "structure_fixtures.json")) as _f:
    FX = json.load(_f)


@pytest.mark.parametrize("idx,ptr", IDX_COMBOS)
@pytest.mark.parametrize("c", FX["matrices"], ids=[c["name"] for c in FX["matrices"]])
def test_reference_cases(c, idx, ptr):
    from sprs_amd.device import DeviceCsMat
    shape, storage = tuple(c["shape"]), c["storage"]
    if c["name"] == "test_new_csr_bad_indptr_length":           # a handle has outer + 1 slice starts by construction: the host refuses
        got = _finding(lambda: DeviceCsMat.new_from_unsorted(shape, np.array(c["indptr"], dtype=ptr), np.array(c["indices"], dtype=idx), c["data"]))
        assert got[:2] == (c["check"]["kind"], c["check"]["text"])
        return
    nnz = len(c["indices"])
    inner, outer = _dims(shape, storage)
    m = _wrap(shape, c["indptr"], c["indices"], c["data"], storage, idx, ptr, nnz=nnz)
    assert _finding(m.check_structure) == (c["check"]["kind"], c["check"]["text"], c["check"]["outer"])
    want = c["from_unsorted"]
    got = []
    assert _finding(lambda: got.append(m.sort_indices())) == (want["kind"], want["text"], want["outer"])
    if want["kind"] == R.OK:
        assert R.same_mat(got[0].to_host(), (shape, c["indptr"], want["indices"], want["data"]))
        made = DeviceCsMat.new_from_unsorted(shape, np.array(c["indptr"], dtype=ptr), np.array(c["indices"], dtype=idx), c["data"], storage=storage)
        assert R.same_mat(made.to_host(), (shape, c["indptr"], want["indices"], want["data"])) and made.storage() == storage
    else:
        assert not got


def test_declared_two_byte_widths_are_inherited():
    from sprs_amd.device import DeviceCsMat
    c = next(c for c in FX["matrices"] if c["name"] == "owned_csr_unsorted_indices")
    m = DeviceCsMat.new_from_unsorted(tuple(c["shape"]), np.array(c["indptr"], dtype=np.uint16), np.array(c["indices"], dtype=np.uint16), c["data"])
    assert m.index_bytes() == 2 and m.indptr_bytes() == 2
    assert R.same_mat(m.to_host(), (c["shape"], c["indptr"], c["from_unsorted"]["indices"], c["from_unsorted"]["data"]))
    t = DeviceCsMat.new_from_unsorted_csc(tuple(c["shape"]), np.array(c["indptr"], dtype=np.uint16), np.array(c["indices"], dtype=np.uint16), c["data"])
    assert t.is_csc() and R.same_mat(t.to_host(), (c["shape"], c["indptr"], c["from_unsorted"]["indices"], c["from_unsorted"]["data"]))


# ---- 2. the length classes: lane groups of 16 / 32 / 64, one wave, one workgroup, the radix route -----------------------------

@pytest.fixture(scope="module")
def seams():
    """(indptr, sorted indices, values): every row a set of distinct indices below 2^14"""
    rng = np.random.default_rng(7)
    ip = np.concatenate([[0], np.cumsum(SEAM_LENGTHS)])
    ix = np.concatenate([np.sort(rng.permutation(SEAM_INNER)[:n]) for n in SEAM_LENGTHS])
    return ip, ix, _special(ix.size, 8)


def _shuffled(seams, keep_every_third):
    ip, ix, dt = seams
    rng = np.random.default_rng(9)
    ix = ix.copy()
    for r, n in enumerate(SEAM_LENGTHS):
        s, e = ip[r], ip[r + 1]
        if keep_every_third and r % 3 == 0:
            continue                               # left sorted: copied, not sorted
        if keep_every_third and n == 1024:
            ix[s:e] = ix[s:e][::-1].copy()         # fully reversed
        elif keep_every_third and n == 4097:
            ix[e - 2:e] = ix[e - 2:e][::-1].copy()  # only its last pair swapped
        else:
            ix[s:e] = rng.permutation(ix[s:e])
    return ip, ix, dt


@pytest.mark.parametrize("storage,idx,ptr", [(CSR,) + w for w in IDX_COMBOS] + [(CSC, np.uint32, np.uint64)])
@pytest.mark.parametrize("partly", [False, True], ids=["all_shuffled", "every_third_sorted"])
def test_class_seams(seams, partly, storage, idx, ptr):
    ip, ix, dt = _shuffled(seams, partly)
    n = len(SEAM_LENGTHS)
    shape = (n, SEAM_INNER) if storage == CSR else (SEAM_INNER, n)
    res = _both(shape, ip, ix, dt, storage, idx, ptr)
    got = res.to_host()
    assert np.array_equal(got[2].astype(np.int64), seams[1])                 # (what the restatement said, said once more)
    assert sorted(got[3].view(np.uint64).tolist()) == sorted(dt.view(np.uint64).tolist())


# ---- 3. tile seams of the check -----------------------------------------------------------------------------------------------

def _tile_case(lengths, inner=1 << 20, seed=3):
    """sorted rows of the given lengths over 3 * TILE + 5 entries: consecutive indices from a random start"""
    assert sum(lengths) == 3 * TILE + 5
    rng = np.random.default_rng(seed)
    ip = np.concatenate([[0], np.cumsum(lengths)])
    ix = np.concatenate([np.arange(n) * 3 + int(rng.integers(1000, 5000)) for n in lengths]) if lengths else np.zeros(0, dtype=np.int64)
    return ip, ix, _special(ix.size, seed + 1), inner


@pytest.mark.parametrize("idx,ptr", IDX_COMBOS)
def test_tile_seam_inside_a_row(idx, ptr):
    """(a) the only violation is the pair at positions TILE - 1 / TILE, inside one row"""
    lengths = [TILE - 20, 50, TILE, TILE - 25]
    ip, ix, dt, inner = _tile_case(lengths)
    assert ip[1] < TILE - 1 and ip[2] > TILE
    ix[TILE - 1], ix[TILE] = ix[TILE], ix[TILE - 1]
    m = _wrap((len(lengths), inner), ip, ix, dt, CSR, idx, ptr)
    assert _finding(m.check_structure) == (R.UNSORTED, "Indices are not sorted", 1)
    _both((len(lengths), inner), ip, ix, dt, CSR, idx, ptr)
    ix[TILE] = ix[TILE - 1]                        # a duplicate across the same seam
    assert _finding(_wrap((len(lengths), inner), ip, ix, dt, CSR, idx, ptr).check_structure) == (R.UNSORTED, "Indices are not sorted", 1)


@pytest.mark.parametrize("idx,ptr", IDX_COMBOS)
def test_tile_seam_between_rows(idx, ptr):
    """(b) a row ends at TILE - 1 and the next starts at TILE with a smaller index: sound"""
    lengths = [TILE, 2 * TILE, 5]
    ip, ix, dt, inner = _tile_case(lengths)
    ix[TILE:3 * TILE] = np.arange(2 * TILE)                    # starts at 0, below everything in front of it
    ix[3 * TILE:] = np.arange(5)
    assert ix[TILE] < ix[TILE - 1] and ix[3 * TILE] < ix[3 * TILE - 1]
    m = _wrap((3, inner), ip, ix, dt, CSR, idx, ptr)
    assert _finding(m.check_structure) == R.GOOD
    res = _both((3, inner), ip, ix, dt, CSR, idx, ptr)
    assert R.same_mat(res.to_host(), ((3, inner), ip, ix, dt))


def test_many_rows_in_one_tile_and_empty_ones():
    """(c) trailing empty rows, more slices in a tile than its LDS table holds (the search falls back to memory), an empty matrix"""
    ones = 3 * TILE + 5
    lengths = [1] * ones
    ip, ix, dt, inner = _tile_case(lengths)
    ip2 = np.concatenate([np.repeat(ip[:-1], 2), [ip[-1]] * 40])            # an empty row in front of every row, 40 more at the end
    shape = (ip2.size - 1, inner)
    assert _finding(_wrap(shape, ip2, ix, dt).check_structure) == R.GOOD
    bad = ix.copy()
    bad[ones - 1] = inner                                                   # the last entry of the last non-empty row
    want = (R.OUT_OF_RANGE, "Indice is larger than inner dimension", 2 * (ones - 1) + 1)
    assert _finding(_wrap(shape, ip2, bad, dt).check_structure) == want == R.check_compressed_structure(inner, shape[0], ip2, bad)
    lengths = [TILE, TILE, TILE, 5]
    ip, ix, dt, inner = _tile_case(lengths)
    ip3 = np.concatenate([ip, [ip[-1]] * 7])
    res = _both((ip3.size - 1, inner), ip3, ix, dt)
    assert R.same_mat(res.to_host(), ((ip3.size - 1, inner), ip3, ix, dt))
    for shape, ipe in (((0, 0), [0]), ((0, 5), [0]), ((4, 0), [0] * 5), ((3, 7), [0] * 4)):
        res = _both(shape, ipe, [], [])
        assert res.nnz() == 0 and res.shape() == shape


# ---- 4. range and precedence ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("idx,ptr", IDX_COMBOS)
def test_range_and_precedence(idx, ptr):
    inner = 100
    ok = ([0, 3, 6], [1, 5, inner - 1, 0, 2, 3], np.arange(6.0))
    assert _finding(_wrap((2, inner), *ok, CSR, idx, ptr).check_structure) == R.GOOD                 # a last index of inner - 1 passes
    assert _finding(_wrap((2, inner), ok[0], [1, 5, inner, 0, 2, 3], ok[2], CSR, idx, ptr).check_structure) == \
        (R.OUT_OF_RANGE, "Indice is larger than inner dimension", 0)
    # a row with both a duplicate and an index >= inner is Unsorted; without the duplicate it is OutOfRange — sorted or not
    for ix, kind in (([inner + 7, 4, 4, 0, 2, 3], R.UNSORTED), ([inner + 7, 4, 5, 0, 2, 3], R.OUT_OF_RANGE),
                     ([4, 5, inner + 7, 0, 2, 3], R.OUT_OF_RANGE), ([4, inner + 7, inner + 7, 0, 2, 3], R.UNSORTED)):
        m = _wrap((2, inner), ok[0], ix, ok[2], CSR, idx, ptr)
        got = _finding(m.sort_indices)
        assert got == R.new_from_unsorted(CSR, (2, inner), ok[0], np.array(ix, dtype=idx), ok[2])[0] and got[::2] == (kind, 0)
    # the lowest offending row decides, whichever kind it holds
    ip = [0, 2, 4, 6, 8]
    low_range = [0, 1, 3, inner, 5, 5, 7, 8]                   # row 1 OutOfRange, row 2 a duplicate
    low_dup = [0, 1, 6, 6, 5, inner, 7, 8]                     # row 1 a duplicate, row 2 OutOfRange
    for ix, want in ((low_range, (R.OUT_OF_RANGE, 1)), (low_dup, (R.UNSORTED, 1))):
        m = _wrap((4, inner), ip, ix, np.arange(8.0), CSR, idx, ptr)
        assert _finding(m.check_structure)[::2] == want and _finding(m.sort_indices)[::2] == want
    _both((4, inner), ip, low_range, np.arange(8.0), CSR, idx, ptr)
    _both((4, inner), ip, [1, 0, 3, inner, 5, 4, 7, 8], np.arange(8.0), CSR, idx, ptr)   # unsorted rows around an out-of-range one


# ---- 5. the indptr pass -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("idx,ptr", IDX_COMBOS)
def test_indptr_findings(idx, ptr):
    """every slice start stays <= the length of the arrays: a check that looked at `indices` anyway would still read inside them"""
    ix, dt = [0, 1, 2, 3, 0, 1], np.arange(6.0)
    cases = [([0, 4, 2, 6], 6, (R.UNSORTED, "Unsorted indptr", R.NO_OUTER)),                          # a decreasing pair
             ([0, 2, 4, 6], 5, (R.SIZE_MISMATCH, "Indices length and inpdtr's nnz do not match", R.NO_OUTER)),   # one above nnz
             ([0, 2, 4, 5], 6, (R.SIZE_MISMATCH, "Indices length and inpdtr's nnz do not match", R.NO_OUTER)),   # one below nnz
             ([0, 6, 5, 6], 6, (R.UNSORTED, "Unsorted indptr", R.NO_OUTER))]
    for ip, nnz, want in cases:
        m = _wrap((3, 8), ip, ix, dt, CSR, idx, ptr, nnz=nnz)
        assert _finding(m.check_structure) == want
        assert _finding(m.sort_indices) == want
        assert R.check_compressed_structure(8, 3, np.array(ip, dtype=ptr), np.array(ix[:nnz], dtype=idx)) == want


def test_indptr_must_start_at_zero_and_widths_are_checked():
    from sprs_amd import SprsHipError, _ffi
    m = _wrap((2, 8), [1, 3, 5], [0, 1, 2, 3], np.arange(4.0), nnz=4)
    with pytest.raises(SprsHipError) as e:
        m.check_structure()
    assert e.value.status == _ffi.INVALID_ARG
    m = _wrap((1, 1 << 33), [0, 1], [5], [1.0], idx=np.uint32, ptr=np.uint32)
    assert _finding(m.check_structure) == (R.OUT_OF_RANGE, "Index type not large enough for this matrix", R.NO_OUTER)
    assert _finding(m.sort_indices) == (R.OUT_OF_RANGE, "Index type not large enough for this matrix", R.NO_OUTER)


# ---- 6. duplicates, 7. the operand -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [5, 20, 40, 700, 3000, 5000])
def test_duplicates_after_the_sort(n):
    """one row per sort route holds two equal indices: no handle, Unsorted, the first such row"""
    rng = np.random.default_rng(n)
    rows = [rng.permutation(1 << 14)[:n] for _ in range(4)]
    rows[2][n // 2] = rows[2][0]
    rows[3][n - 1] = rows[3][1]
    ip = np.arange(5) * n
    m = _wrap((4, 1 << 14), ip, np.concatenate(rows), _special(4 * n, n))
    got = []
    assert _finding(lambda: got.append(m.sort_indices())) == (R.UNSORTED, "Indices are not sorted", 2) and not got
    assert R.new_from_unsorted(CSR, (4, 1 << 14), ip, np.concatenate(rows), np.zeros(4 * n))[0] == (R.UNSORTED, "Indices are not sorted", 2)


def test_operand_untouched(seams):
    ip, ix, dt = _shuffled(seams, True)
    from sprs_amd.device import DeviceCsMat
    shape = (len(SEAM_LENGTHS), SEAM_INNER)
    m = DeviceCsMat.from_host(shape, ip.astype(np.uint64), ix.astype(np.uint64), dt, validate=False)
    before = m.to_host()
    res = m.sort_indices()
    assert R.same_mat(m.to_host(), before) and R.same_mat(before, (shape, ip, ix, dt))
    assert R.same_mat(res.to_host(), (shape, ip, seams[1], res.to_host()[3]))
    again = res.sort_indices()                     # a valid operand: the copy is the result
    assert R.same_mat(again.to_host(), res.to_host())


# ---- 8. vectors ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("idx", [np.uint64, np.uint32])
@pytest.mark.parametrize("n", [0, 1, 2, 64, 65, 4096, 4097, 70000])
def test_vectors(n, idx):
    """up to 4096 entries one workgroup sorts in LDS, longer vectors go through the radix sort (70000 is also above the size up
    to which an upload is checked on the host)"""
    from sprs_amd.device import DeviceCsVec
    rng = np.random.default_rng(n + 1)
    dim = max(4 * n, 10)
    ix = rng.permutation(dim)[:n]
    dt = _special(n, n)
    v = _wrap_vec(dim, ix, dt, idx)
    want, ref = R.vec_new_from_unsorted(dim, ix.astype(idx), dt)
    assert want == R.GOOD and _finding(v.check_structure) == R.check_vec(dim, ix.astype(idx))
    res = v.sort_indices()
    got = res.to_host()
    assert got[0] == dim and res.index_bytes() == np.dtype(idx).itemsize
    assert np.array_equal(got[1].astype(np.uint64), ref[1].astype(np.uint64)) and np.array_equal(got[2].view(np.uint64), ref[2].view(np.uint64))
    assert _finding(res.check_structure) == R.GOOD
    back = v.to_host()                             # the operand is only read
    assert np.array_equal(back[1].astype(np.int64), ix) and np.array_equal(back[2].view(np.uint64), dt.view(np.uint64))
    made = DeviceCsVec.new_from_unsorted(dim, ix.astype(idx), dt).to_host()
    assert np.array_equal(made[1], got[1]) and np.array_equal(made[2].view(np.uint64), got[2].view(np.uint64))


@pytest.mark.parametrize("n", [6, 5000])
def test_vector_findings(n):
    rng = np.random.default_rng(n)
    dim = 4 * n
    ix = rng.permutation(dim)[:n]
    dt = np.arange(float(n))
    dup = ix.copy()
    dup[n - 1] = dup[0]
    far = np.sort(ix)
    far[-1] = dim                                  # sorted, its last index == dim: the first check's finding
    mixed = ix.copy()
    mixed[0] = dim                                 # unsorted and out of range: sorted first, then SizeMismatch
    huge = ix.astype(np.uint64)
    huge[1] = (1 << 63) + 5                        # no packed key holds this one
    for arr, want in ((dup, (R.UNSORTED, "Unsorted indices", 0)), (far, (R.SIZE_MISMATCH, "indices larger than vector size", 0)),
                      (mixed, (R.SIZE_MISMATCH, "indices larger than vector size", 0)), (huge, (R.SIZE_MISMATCH, "indices larger than vector size", 0))):
        v = _wrap_vec(dim, arr, dt)
        assert R.vec_new_from_unsorted(dim, arr, dt)[0] == want
        got = []
        assert _finding(lambda: got.append(v.sort_indices())) == want and not got
        assert _finding(v.check_structure) == R.check_vec(dim, arr)
    assert _finding(_wrap_vec(dim, np.sort(ix), dt).check_structure) == R.GOOD


# ---- 9. torch tensors ----------------------------------------------------------------------------------------------------------

def _torch():
    if EMULATED:
        pytest.skip("torch tensors live on a real device")
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    return torch


@pytest.mark.parametrize("itype", ["int64", "int32"])
def test_wrap_torch_validates(itype):
    torch = _torch()
    from sprs_amd.device import DeviceCsMat, DeviceCsVec
    t = getattr(torch, itype)
    ip = torch.tensor([0, 2, 4, 5], dtype=t, device="cuda")
    dt = torch.arange(5, dtype=torch.float64, device="cuda")
    good = torch.tensor([0, 3, 1, 2, 3], dtype=t, device="cuda")
    m = DeviceCsMat.wrap_torch((3, 4), ip, good, dt, validate=True)
    assert m.nnz() == 5
    for ix, want in (([0, 3, 2, 1, 3], (R.UNSORTED, "Indices are not sorted", 1)), ([0, 3, 1, -1, 3], (R.OUT_OF_RANGE, "Indice is larger than inner dimension", 1)),
                     ([0, 3, 1, 2, 4], (R.OUT_OF_RANGE, "Indice is larger than inner dimension", 2))):
        bad = torch.tensor(ix, dtype=t, device="cuda")
        assert _finding(lambda: DeviceCsMat.wrap_torch((3, 4), ip, bad, dt, validate=True)) == want
        assert DeviceCsMat.wrap_torch((3, 4), ip, bad, dt).nnz() == 5            # the default stays new_trusted
    v = DeviceCsVec.borrow(9, good[2:], dt[2:], validate=True)
    assert v.nnz() == 3
    assert _finding(lambda: DeviceCsVec.borrow(9, good[:3], dt[:3], validate=True)) == (R.UNSORTED, "Unsorted indices", 0)
    assert _finding(lambda: DeviceCsVec.borrow(3, good[2:], dt[2:], validate=True)) == (R.SIZE_MISMATCH, "indices larger than vector size", 0)


def test_sorted_wrapped_matrix_multiplies_like_the_sorted_upload(seams):
    torch = _torch()
    from sprs_amd.device import DeviceCsMat, DeviceVec
    ip, ix, _ = _shuffled(seams, False)
    rng = np.random.default_rng(11)
    dt = rng.standard_normal(ix.size)
    shape = (len(SEAM_LENGTHS), SEAM_INNER)
    tip, tix = torch.tensor(ip, dtype=torch.int64, device="cuda"), torch.tensor(ix, dtype=torch.int64, device="cuda")
    tdt = torch.tensor(dt, dtype=torch.float64, device="cuda")
    res = DeviceCsMat.wrap_torch(shape, tip, tix, tdt).sort_indices()
    _, sorted_mat = R.new_from_unsorted(CSR, shape, ip, ix, dt)
    up = DeviceCsMat.from_host(shape, ip.astype(np.uint64), sorted_mat[2], sorted_mat[3])
    x = DeviceVec.from_host(rng.standard_normal(SEAM_INNER))
    assert np.array_equal((res * x).to_host().view(np.uint64), (up * x).to_host().view(np.uint64))
