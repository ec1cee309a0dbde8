"""Device construction — kronecker_product, same_storage_fast_stack, vstack, hstack, bmat (sprs/src/sparse/kronecker.rs,
construct.rs) — bit for bit against tests/construct_ref.py: indptr, indices and the uint64 view of the values, no tolerance
anywhere.

The small cases also run against the kernel emulator (tests/test_construct_emu_cpu.py); the large and the torch cases need a
real device."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import construct_ref as R
from conftest import IDX_COMBOS, ROOT
from helpers import fresh_blocks, ragged_csr

pytestmark = pytest.mark.gpu

EMULATED = bool(os.environ.get("SPRS_HIP_LIBRARY"))
CSR, CSC = R.CSR, R.CSC
# (index, indptr): the four pairs the kernels are compiled for and the 2-byte declared widths (kept as 4 bytes on the device)
WIDTHS = IDX_COMBOS + [(np.uint64, np.uint32), (np.uint16, np.uint16)]
PAIRINGS = [(CSR, CSR), (CSR, CSC), (CSC, CSC), (CSC, CSR)]
NAN_PAYLOAD = 0x7FF8000000ABCDEF


@pytest.fixture(scope="module", autouse=True)
def _need_device():
    import sprs_amd
    if sprs_amd.device_count() < 1:
        pytest.skip("no HIP device")


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(ROOT, "tests", "golden", "construct_fixtures.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def tile():
    import sprs_amd
    return int(sprs_amd.get_option("construct_tile"))


def fmat(d):
    return R.mat(d["storage"], d["shape"], d["indptr"], d["indices"], d["data"])


def dev(m, idx=np.uint64, ptr=np.uint64):
    from sprs_amd.device import DeviceCsMat
    m = R.to_owned(m)
    return DeviceCsMat.from_host(m[1], m[2].astype(ptr), m[3].astype(idx), m[4], storage=m[0])


def host(res):
    shape, ip, ix, dt = res.to_host()
    return (res.storage(), shape, ip, ix, dt)


def check(res, want):
    got = host(res)
    assert R.same_mat(got, want)
    assert int(got[2][0]) == 0 and int(got[2][-1]) == got[3].size == got[4].size == res.nnz()   # a proper indptr, exact nnz


def ragged(lens, inner, seed, storage=CSR, special=False):
    """outer slices of the given lengths; storage CSC: the same arrays as the columns of an inner x len(lens) matrix"""
    shape, ip, ix, dt = ragged_csr(np.asarray(lens, dtype=np.int64), inner, seed=seed, positive=False)
    if special:
        dt = _special(dt, seed)
    m = R.mat(CSR, shape, ip, ix, dt)
    return m if storage == CSR else R.transpose(m)


def _special(dt, seed):
    """-0.0, a stored 0.0 and inf among the values"""
    rng = np.random.default_rng(seed)
    dt = np.array(dt, dtype=np.float64)
    dt[rng.random(dt.size) < 0.1] = -0.0
    dt[rng.random(dt.size) < 0.1] = 0.0
    dt[rng.random(dt.size) < 0.1] = np.inf
    dt[rng.random(dt.size) < 0.05] = -np.inf
    return dt


def lens_with_sum(total, rows, seed, longest=None, cap=None):
    """`rows` ragged lengths (a third of them 0 where `cap`, the longest a slice may be, allows) that sum to `total`"""
    rng = np.random.default_rng(seed)
    lens = np.zeros(rows, dtype=np.int64)
    live = np.flatnonzero(rng.random(rows) >= 0.3)
    if live.size == 0:
        live = np.array([rows // 2])
    if longest:
        lens[live[0]] = longest
    for _ in range(total - int(lens.sum())):
        room = live if cap is None else live[lens[live] < cap]
        if room.size == 0:
            room = np.flatnonzero(lens < cap)
        lens[room[rng.integers(0, room.size)]] += 1
    assert lens.sum() == total
    return lens


def kron(a, b, stream=None):
    from sprs_amd import construct
    fresh_blocks()
    return construct.kronecker_product(a, b, stream=stream)


# ---- Kronecker product ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("idx,ptr", WIDTHS)
@pytest.mark.parametrize("sa,sb", PAIRINGS)
def test_kron_golden(fx, sa, sb, idx, ptr):
    """test_kronecker_product (kronecker.rs:101-152) in its four storage pairings and every width pair"""
    from test_construct_cpu import entries, from_triplets
    c = fx["kronecker"]
    a, b = from_triplets(c["a"]["shape"], c["a"]["triplets"], sa), from_triplets(c["b"]["shape"], c["b"]["triplets"], sb)
    res = kron(dev(a, idx, ptr), dev(b, idx, ptr))
    check(res, R.kronecker_product(a, b))
    assert res.storage() == sa and res.shape() == (6, 6)
    assert entries(host(res)) == {(r, col): float(v) for r, col, v in c["expected"]}
    assert res.index_bytes() == np.dtype(idx).itemsize and res.indptr_bytes() == np.dtype(ptr).itemsize


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_kron_result_sizes_at_the_tile(tile, delta):
    """nnz(a) * nnz(b) = T - 1, T, T + 1"""
    n = tile + delta
    na = next(d for d in range(int(n ** 0.5), 0, -1) if n % d == 0)
    a = ragged(lens_with_sum(na, 6, 1), 50, 1)
    b = ragged(lens_with_sum(n // na, 9, 2), 3000 // 4, 2)
    res = kron(dev(a), dev(b))
    assert res.nnz() == n
    check(res, R.kronecker_product_vec(a, b))


def test_kron_one_slice_over_several_tiles(tile):
    """a 70-entry row (x) a 70-entry row is one result slice of 4900 entries: more than two tiles at T = 2048"""
    k = 70
    assert k * k > 2 * tile
    a = ragged([3, 0, k, 2], 90, 3)
    b = ragged([1, k, 0, 4], 80, 4)
    check(kron(dev(a), dev(b)), R.kronecker_product_vec(a, b))


def test_kron_runs_of_empty_slices(tile):
    """empty rows of a and of b at the front, in the middle and at the end; the slice (2, 1) ends exactly at the first tile
    edge and a run of empty slices starts there"""
    a = ragged([0, 0, 32, 0, 0, 0, 5, 0, 0], 40, 5)
    b = ragged([0, tile // 32, 0, 0, 0, 7, 0, 0], 100, 6)
    want = R.kronecker_product_vec(a, b)
    assert int(want[2][2 * 8 + 2]) == tile and int(want[2][2 * 8 + 5]) == tile
    check(kron(dev(a), dev(b)), want)
    assert R.same_mat(want, R.kronecker_product(a, b))
    check(kron(dev(b), dev(a)), R.kronecker_product_vec(b, a))


def test_kron_row_lengths_of_b_around_the_wave():
    a = ragged([2, 0, 3, 1], 9, 7)
    b = ragged([1, 63, 64, 65, 0, 1], 70, 8)
    check(kron(dev(a), dev(b)), R.kronecker_product_vec(a, b))
    check(kron(dev(b), dev(a)), R.kronecker_product_vec(b, a))


@pytest.mark.parametrize("idx,ptr", WIDTHS)
def test_kron_empty_operands(idx, ptr):
    """nnz(a) = 0, nnz(b) = 0 and a 0-row operand: the indptr has its full length and is all zeros"""
    full = ragged([2, 0, 3], 5, 9)
    none = ragged([0, 0, 0, 0], 6, 9)
    norow = R.mat(CSR, (0, 4), [0], [], [])
    for a, b in ((none, full), (full, none), (none, none), (norow, full), (full, norow)):
        res = kron(dev(a, idx, ptr), dev(b, idx, ptr))
        got = host(res)
        assert got[1] == (a[1][0] * b[1][0], a[1][1] * b[1][1]) and res.nnz() == 0
        assert got[2].size == a[1][0] * b[1][0] + 1 and not got[2].any()
        check(res, R.kronecker_product(a, b))


@pytest.mark.parametrize("idx,ptr", WIDTHS)
@pytest.mark.parametrize("sa,sb", PAIRINGS)
def test_kron_non_square_storage_pairings(sa, sb, idx, ptr):
    """a is 5 x 9 and b 7 x 4: a transposition slip changes the shape or the indices; the result has a's storage"""
    a = ragged(lens_with_sum(17, 5 if sa == CSR else 9, 10, cap=9 if sa == CSR else 5), 9 if sa == CSR else 5, 10, sa)
    b = ragged(lens_with_sum(11, 7 if sb == CSR else 4, 11, cap=4 if sb == CSR else 7), 4 if sb == CSR else 7, 11, sb)
    assert a[1] == (5, 9) and b[1] == (7, 4)
    res = kron(dev(a, idx, ptr), dev(b, idx, ptr))
    assert res.storage() == sa and res.shape() == (35, 36)
    check(res, R.kronecker_product(a, b))
    assert res.index_bytes() == np.dtype(idx).itemsize and res.indptr_bytes() == np.dtype(ptr).itemsize


def test_kron_special_values():
    """-0.0, a stored 0.0, +-inf on both sides (inf * 0.0 is the reference's NaN), a NaN with a payload on one side: nothing
    is dropped, bits are compared"""
    a = ragged(lens_with_sum(40, 8, 12), 30, 12, special=True)
    b = ragged(lens_with_sum(60, 9, 13), 30, 13, special=True)
    a[4].view(np.uint64)[[3, 17]] = NAN_PAYLOAD
    a[4][:3] = [-0.0, 0.0, np.inf]
    b[4][:3] = [np.inf, -0.0, 0.0]
    want = R.kronecker_product_vec(a, b)
    assert R.same_mat(want, R.kronecker_product(a, b))
    made = R.bits(want[4]) == 0xFFF8000000000000                    # inf * 0.0 on the reference's hardware: its default NaN
    assert made.sum() > 2 and (R.bits(want[4]) == NAN_PAYLOAD).sum() > 2 and (want[4] == 0).sum() > 2 and np.isinf(want[4]).sum() > 2
    for sa, sb in PAIRINGS:
        x = a if sa == CSR else R.to_other_storage(a)
        y = b if sb == CSR else R.to_other_storage(b)
        check(kron(dev(x), dev(y)), R.kronecker_product(x, y))


def test_kron_sliced_operand():
    """operands cut by the device slice_outer"""
    a = ragged(lens_with_sum(60, 12, 14), 20, 14)
    b = ragged(lens_with_sum(50, 10, 15), 20, 15)
    da, db = dev(a).slice_outer(3, 9), dev(b).slice_outer(2, 10)
    cut = lambda m, s, e: (m[0], (e - s, m[1][1]), m[2][s:e + 1], m[3][m[2][s]:m[2][e]], m[4][m[2][s]:m[2][e]])
    check(kron(da, db), R.kronecker_product(cut(a, 3, 9), cut(b, 2, 10)))


def _raw_kron(a, b):
    from sprs_amd import _ffi
    h = C.c_void_p(0xDEAD)
    st = _ffi.lib.sprs_hip_csmat_kronecker_f64(a._h, b._h, C.byref(h), None)
    return st, h.value, _ffi.lib.sprs_hip_last_error().decode()


def test_kron_overflow_is_decided_by_shape():
    from sprs_amd import _ffi
    # 4-byte indices: inner(a) * inner(b) = 65536 * 65537, no entry stored
    a = R.mat(CSR, (1, 65536), [0, 0], [], [])
    b = R.mat(CSR, (1, 65537), [0, 0], [], [])
    st, h, msg = _raw_kron(dev(a, np.uint32, np.uint64), dev(b, np.uint32, np.uint64))
    assert st == _ffi.INDEX_OVERFLOW and h == 0xDEAD and "not large enough" in msg
    b2 = R.mat(CSR, (1, 65536), [0, 0], [], [])                      # 2^32 columns: the last index is 2^32 - 1 and fits
    st, h, _ = _raw_kron(dev(a, np.uint32, np.uint64), dev(b2, np.uint32, np.uint64))
    assert st == _ffi.OK
    _ffi.check(_ffi.lib.sprs_hip_csmat_free(C.c_void_p(h)))
    # the same decision in the other storage and for the 2-byte declared width
    st, h, _ = _raw_kron(dev(R.transpose(a), np.uint32, np.uint64), dev(R.transpose(b), np.uint32, np.uint64))
    assert st == _ffi.INDEX_OVERFLOW and h == 0xDEAD
    st, h, _ = _raw_kron(dev(R.mat(CSR, (1, 256), [0, 0], [], []), np.uint16, np.uint16), dev(R.mat(CSR, (1, 257), [0, 0], [], []), np.uint16, np.uint16))
    assert st == _ffi.INDEX_OVERFLOW and h == 0xDEAD
    # 4-byte indptr: nnz(a) = nnz(b) = 65536
    row = R.mat(CSR, (1, 65536), [0, 65536], np.arange(65536), np.ones(65536))
    d = dev(row, np.uint64, np.uint32)
    st, h, msg = _raw_kron(d, d)
    assert st == _ffi.INDEX_OVERFLOW and h == 0xDEAD and "nnz" in msg
    # operands of different index types: the status of csmat_binop
    st, h, msg = _raw_kron(dev(a, np.uint32, np.uint64), dev(b, np.uint64, np.uint64))
    assert st == _ffi.STORAGE_MISMATCH and h == 0xDEAD and "index types" in msg


# ---- stacking ------------------------------------------------------------------------------------------------------------------

def stack(name, mats, stream=None):
    from sprs_amd import construct
    fresh_blocks()
    return getattr(construct, name)(mats, stream=stream)


@pytest.mark.parametrize("idx,ptr", WIDTHS)
def test_stacking_golden(fx, idx, ptr):
    """construct.rs:198-319 through the device"""
    up = lambda m: dev(m, idx, ptr)
    a, b = fmat(fx["mat1"]), fmat(fx["mat2"])
    want = fmat(fx["mat1_vstack_mat2"])
    check(stack("same_storage_fast_stack", [up(a), up(b)]), want)
    check(stack("vstack", [up(a), up(b)]), want)
    check(stack("hstack", [up(R.transpose(a)), up(R.transpose(b))]), R.transpose(want))
    res = stack("vstack", [up(R.to_csc(a)), up(b)])
    check(res, want)
    assert res.index_bytes() == np.dtype(idx).itemsize and res.indptr_bytes() == np.dtype(ptr).itemsize
    c = fx["bmat_simple"]
    e5, e4 = (up(R.eye(n)) for n in c["eye"])
    check(stack("bmat", [[e5, None], [None, e4]]), fmat(c["expected"]))
    for c in fx["bmat_complex"]:
        blocks = [[None if name is None else up(fmat(fx[name])) for name in row] for row in c["blocks"]]
        check(stack("bmat", blocks), fmat(c["expected"]))


def test_stacking_one_block():
    a = ragged(lens_with_sum(30, 7, 20), 11, 20)
    at = R.to_other_storage(a)
    for name, ref in (("same_storage_fast_stack", R.same_storage_fast_stack), ("vstack", R.vstack), ("hstack", R.hstack)):
        check(stack(name, [dev(a)]), ref([a]))
        check(stack(name, [dev(at)]), ref([at]))
    check(stack("bmat", [[dev(a)]]), R.bmat([[a]]))
    check(stack("bmat", [[dev(at)]]), R.bmat([[at]]))


def test_bmat_many_small_blocks():
    """a 40 x 40 bmat of 3 x 3 blocks with a checkerboard of None: 800 blocks, one launch"""
    kinds = [ragged(lens_with_sum(n, 3, 30 + n, cap=3), 3, 30 + n, CSR if n % 2 else CSC) for n in range(0, 9)]
    handles = [dev(k) for k in kinds]
    pick = lambda i, j: None if (i + j) % 2 else (i * 7 + j * 3) % len(kinds)
    grid = [[pick(i, j) for j in range(40)] for i in range(40)]
    res = stack("bmat", [[None if k is None else handles[k] for k in row] for row in grid])
    assert res.shape() == (120, 120)
    check(res, R.bmat_vec([[None if k is None else kinds[k] for k in row] for row in grid]))
    small = [row[:4] for row in grid[:4]]
    assert R.same_mat(R.bmat_vec([[None if k is None else kinds[k] for k in row] for row in small]),
                      R.bmat([[None if k is None else kinds[k] for k in row] for row in small]))


def test_vstack_empty_blocks_in_the_middle():
    """a block without entries and a block with 0 rows between two others"""
    a = ragged(lens_with_sum(20, 5, 40), 8, 40)
    none = ragged([0, 0, 0], 8, 41)
    norow = R.mat(CSR, (0, 8), [0], [], [])
    b = ragged(lens_with_sum(15, 4, 42), 8, 42)
    mats = [a, none, norow, b, norow]
    check(stack("vstack", [dev(m) for m in mats]), R.vstack(mats))
    check(stack("hstack", [dev(R.transpose(m)) for m in mats]), R.hstack([R.transpose(m) for m in mats]))
    check(stack("bmat", [[dev(m)] for m in mats]), R.bmat([[m] for m in mats]))
    check(stack("vstack", [dev(norow), dev(norow)]), R.vstack([norow, norow]))


def test_stacking_block_sizes_at_the_tile(tile):
    """blocks of T - 1, T and T + 1 entries, alone in their super-row (vstack) and side by side (bmat)"""
    mats = [ragged(lens_with_sum(tile + d, 30, 50 + d, longest=300), 400, 50 + d) for d in (-1, 0, 1)]
    check(stack("vstack", [dev(m) for m in mats]), R.vstack_vec(mats))
    check(stack("bmat", [[dev(m) for m in mats], [dev(mats[2]), None, dev(mats[0])]]), R.bmat_vec([mats, [mats[2], None, mats[0]]]))
    check(stack("hstack", [dev(R.transpose(m)) for m in mats]), R.hstack_vec([R.transpose(m) for m in mats]))


def test_bmat_tile_over_a_long_run_of_empty_slices():
    """one tile of a block that shares its super-row meets more slices than the kernel keeps in LDS (2500 empty ones between two
    short ones): the slice starts are read from memory there"""
    lens = np.zeros(3000, dtype=np.int64)
    lens[[0, 2501, 2999]] = [5, 4, 3]
    a = ragged(lens, 9, 55)
    lens_b = np.zeros(3000, dtype=np.int64)
    lens_b[[1, 1200, 2501]] = [2, 6, 1]
    b = ragged(lens_b, 7, 56)
    check(stack("bmat", [[dev(a), dev(b)]]), R.bmat_vec([[a, b]]))
    check(stack("hstack", [dev(a), dev(b)]), R.hstack_vec([a, b]))


def test_stacking_mixed_storages():
    a = ragged(lens_with_sum(40, 9, 60), 12, 60, special=True)
    b = ragged(lens_with_sum(25, 6, 61), 12, 61)
    c = ragged(lens_with_sum(33, 9, 62, cap=5), 5, 62)
    bt, ct = R.to_other_storage(b), R.to_other_storage(c)
    for mats in ([a, bt, b], [bt, bt], [bt, a]):
        res = stack("vstack", [dev(m) for m in mats])
        assert res.storage() == CSR
        check(res, R.vstack(mats))
    for mats in ([a, ct], [c, a], [ct, R.to_other_storage(a), c]):
        res = stack("hstack", [dev(m) for m in mats])
        assert res.storage() == CSC
        check(res, R.hstack(mats))
    blocks = [[a, ct], [None, R.transpose(ragged(lens_with_sum(7, 5, 63, cap=4), 4, 63))]]
    res = stack("bmat", [[None if m is None else dev(m) for m in row] for row in blocks])
    assert res.storage() == CSR
    check(res, R.bmat(blocks))


def test_bmat_unaligned_blocks():
    """super-rows [2 | 3] over [3 | 2] columns: accepted, the offset of a block is the sum of the ACTUAL widths to its left"""
    blk = lambda r, c, seed: ragged(lens_with_sum(r + c, r, seed, cap=c), c, seed)
    blocks = [[blk(2, 2, 70), blk(2, 3, 71)], [blk(3, 3, 72), blk(3, 2, 73)]]
    res = stack("bmat", [[dev(m) for m in row] for row in blocks])
    assert res.shape() == (5, 5)
    check(res, R.bmat(blocks))
    # a None takes the column's maximum: [None | 2] over [3 | 2] is 5 wide in both super-rows
    blocks = [[None, blk(2, 2, 74)], [blk(3, 3, 75), blk(3, 2, 76)]]
    check(stack("bmat", [[None if m is None else dev(m) for m in row] for row in blocks]), R.bmat(blocks))


def _fails(name, mats, status, text):
    from sprs_amd import SprsHipError
    with pytest.raises(SprsHipError) as e:
        stack(name, mats)
    assert e.value.status == status and str(e.value).endswith(text), str(e.value)


def test_stacking_errors_in_the_reference_order(fx):
    from sprs_amd import _ffi
    a, c, d = fmat(fx["mat1"]), fmat(fx["mat3"]), fmat(fx["mat4"])
    da, dc, dd = dev(a), dev(c), dev(d)
    for ref, args in ((R.same_storage_fast_stack, [a, c]), (R.same_storage_fast_stack, [a, d]), (R.same_storage_fast_stack, [a, R.transpose(c)]),
                      (R.vstack, [a, c]), (R.hstack, [a, R.transpose(c)])):
        with pytest.raises(AssertionError):
            ref(args)
    _fails("same_storage_fast_stack", [], _ffi.INVALID_ARG, "Empty stacking list")
    _fails("same_storage_fast_stack", [da, dc], _ffi.DIM_MISMATCH, "Dimension mismatch")
    _fails("same_storage_fast_stack", [da, dd], _ffi.STORAGE_MISMATCH, "Storage mismatch")
    _fails("same_storage_fast_stack", [da, dev(R.transpose(c))], _ffi.DIM_MISMATCH, "Dimension mismatch")   # both wrong: the dimensions first
    _fails("vstack", [], _ffi.INVALID_ARG, "Empty stacking list")
    _fails("hstack", [], _ffi.INVALID_ARG, "Empty stacking list")
    _fails("vstack", [da, dc], _ffi.DIM_MISMATCH, "Dimension mismatch")
    _fails("vstack", [dd, dc], _ffi.DIM_MISMATCH, "Dimension mismatch")
    _fails("hstack", [da, dev(R.transpose(c))], _ffi.DIM_MISMATCH, "Dimension mismatch")
    _fails("vstack", [da, dev(a, np.uint32, np.uint64)], _ffi.STORAGE_MISMATCH, "index types (construct.rs:10-17)")
    # bmat: the list's shape, empty row, empty column, then the dimensions (construct.rs:104-123, hstack, vstack)
    _fails("bmat", [], _ffi.INVALID_ARG, "Empty stacking list")
    _fails("bmat", [[]], _ffi.INVALID_ARG, "Empty stacking list")
    _fails("bmat", [[None, None], [None]], _ffi.DIM_MISMATCH, "Dimension mismatch")
    _fails("bmat", [[None, None], [da, dc]], _ffi.INVALID_ARG, "Empty bmat row")
    _fails("bmat", [[dc, None], [da, None]], _ffi.INVALID_ARG, "Empty bmat col")
    _fails("bmat", [[None, None], [da, None]], _ffi.INVALID_ARG, "Empty bmat row")                # an empty row AND an empty column
    _fails("bmat", [[da, dev(R.zero((4, 2)))]], _ffi.DIM_MISMATCH, "Dimension mismatch")          # rows differ inside a super-row
    _fails("bmat", [[da], [dc]], _ffi.DIM_MISMATCH, "Dimension mismatch")                         # total columns differ
    _fails("bmat", [[da, dev(a, np.uint32, np.uint32)]], _ffi.STORAGE_MISMATCH, "index types (construct.rs:94-102)")
    for bad in ([[None, None], [a, c]], [[c, None], [a, None]], [[a, R.zero((4, 2))]], [[a], [c]]):
        with pytest.raises(AssertionError):
            R.bmat(bad)


def test_vstack_puts_slice_outer_cuts_back_together():
    """the inverse of slice_outer: the cuts of a ragged matrix at 3 points, stacked, are the matrix bit for bit"""
    m = ragged(lens_with_sum(3000, 64, 80, longest=900), 1200, 80, special=True)
    m[4].view(np.uint64)[5] = NAN_PAYLOAD
    for storage, name in ((CSR, "vstack"), (CSC, "hstack")):
        x = m if storage == CSR else R.transpose(m)
        d = dev(x, np.uint32, np.uint64)
        cuts = [0, 17, 18, 40, 64]
        parts = [d.slice_outer(s, e) for s, e in zip(cuts[:-1], cuts[1:])]
        check(stack(name, parts), x)
        check(stack("same_storage_fast_stack", parts), x)


# ---- end to end ----------------------------------------------------------------------------------------------------------------

def _tridiag(n):
    lens = np.full(n, 3)
    lens[[0, -1]] = 2
    ip = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=ip[1:])
    ix = np.concatenate([[c for c in (r - 1, r, r + 1) if 0 <= c < n] for r in range(n)])
    dt = np.where(ix == np.repeat(np.arange(n), lens), 2.0, -1.0)
    return R.mat(CSR, (n, n), ip, ix, dt)


def test_grid_laplacian_end_to_end():
    """kron(I, T) + kron(T, I) for a 33 x 33 grid through the device product and the device add, against the same expression
    in construct_ref + binop_ref; y = A x on the result against the oracle (small integers: exact, so equal)"""
    import binop_ref as B
    from oracle import oracle
    from sprs_amd.device import DeviceVec
    n = 33
    t, eye = _tridiag(n), R.eye(n)
    dt_, de = dev(t), dev(eye)
    lap = kron(de, dt_) + kron(dt_, de)
    k1, k2 = R.kronecker_product(eye, t), R.kronecker_product(t, eye)
    want = B.csmat_binop_ref(k1[1:], k2[1:], B.ADD)
    check(lap, (CSR,) + tuple(want))
    assert lap.nnz() == 5 * n * n - 4 * n
    x = np.arange(n * n, dtype=np.float64) % 17 - 8
    y = (lap * DeviceVec.from_host(x)).to_host()
    y_ref = np.zeros(n * n)
    oracle.mul_acc_mat_vec_csr(want[0], want[1].astype(np.uint64), want[2].astype(np.uint64), want[3], x, y_ref)
    assert np.array_equal(y, y_ref)


# ---- real device only ----------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(EMULATED, reason="torch streams: real device only")
def test_non_blocking_stream():
    """the operands are written on a non-blocking torch stream and used there with no host synchronise in between; the results
    are downloaded straight away"""
    import torch
    from sprs_amd.device import DeviceCsMat
    a = ragged(lens_with_sum(300, 40, 90), 64, 90)
    b = ragged(lens_with_sum(200, 25, 91), 64, 91)
    devc = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=devc)
    with torch.cuda.stream(s):
        t = []
        for m in (a, b):
            t.append(tuple(torch.zeros(arr.size, dtype=tt, device=devc) for arr, tt in ((m[2], torch.int64), (m[3], torch.int64), (m[4], torch.float64))))
        torch.cuda._sleep(20_000_000)                  # keep the stream busy: the copies below land late
        for m, arrs in zip((a, b), t):
            for dst, src in zip(arrs, m[2:]):
                dst.copy_(torch.from_numpy(src).to(devc, non_blocking=True))
        da, db = (DeviceCsMat.wrap_torch(m[1], *arrs) for m, arrs in zip((a, b), t))
        k = kron(da, db, stream=s)
        v = stack("vstack", [da, db, da], stream=s)
        bm = stack("bmat", [[da, None], [db, db]], stream=s)
    check(k, R.kronecker_product_vec(a, b))
    check(v, R.vstack_vec([a, b, a]))
    check(bm, R.bmat_vec([[a, None], [b, b]]))


@pytest.mark.skipif(EMULATED, reason="large operands: real device only")
def test_kron_hub_rows_3000():
    """two 3000-row ragged matrices with a hub row each: the hub (x) hub slice alone is 10^6 entries"""
    rng = np.random.default_rng(100)
    lens_a, lens_b = (rng.random(3000) < 0.66).astype(np.int64), (rng.random(3000) < 0.66).astype(np.int64)
    lens_a[1234], lens_b[77] = 1000, 1000
    a, b = ragged(lens_a, 5000, 101), ragged(lens_b, 4000, 102)
    res = kron(dev(a, np.uint32, np.uint64), dev(b, np.uint32, np.uint64))
    assert res.nnz() == R.nnz(a) * R.nnz(b) > 8 * 10 ** 6
    check(res, R.kronecker_product_vec(a, b))
