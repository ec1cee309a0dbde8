"""Device sparse binops — `&A + &B`, `&A - &B`, binop::mul_mat_same_storage, `&A * s`, `&v + &w`, `&v - &w`
(sprs/src/sparse/binop.rs:20-271, 435-479; vec.rs:1133-1226) — bit for bit: indptr, indices and value bits, no tolerance.

The small cases also run against the kernel emulator (tests/test_binop_emu_cpu.py); the large and the torch cases need a real
device."""
import json
import os

import numpy as np
import pytest

from binop_ref import ADD, MUL, SUB, bits, csmat_binop_ref, csmat_binop_vec, csvec_binop_ref, csvec_binop_vec, same_mat, same_vec
from conftest import IDX_COMBOS, ROOT, as_csr
from helpers import ragged_csr

pytestmark = pytest.mark.gpu

EMULATED = bool(os.environ.get("SPRS_HIP_LIBRARY"))
OPS = [ADD, SUB, MUL]
WIDTHS = IDX_COMBOS + [(np.uint16, np.uint16)]


@pytest.fixture(scope="module", autouse=True)
def _need_device():
    import sprs_amd
    if sprs_amd.device_count() < 1:
        pytest.skip("no HIP device")


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(ROOT, "tests", "golden", "binop_fixtures.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def tile():
    import sprs_amd
    return int(sprs_amd.get_option("binop_tile"))


def _mat(m, storage=0, idx=np.uint64, ptr=np.uint64):
    from sprs_amd.device import DeviceCsMat
    shape, ip, ix, dt = m
    return DeviceCsMat.from_host(tuple(shape), np.asarray(ip).astype(ptr), np.asarray(ix).astype(idx), np.asarray(dt, dtype=np.float64),
                                 storage=storage)


def _vec(v, dtype=np.uint64):
    from sprs_amd.device import DeviceCsVec
    dim, idx, val = v
    return DeviceCsVec.from_host(dim, np.asarray(idx, dtype=dtype), np.asarray(val, dtype=np.float64))


def _fxvec(d):
    return d["dim"], d["indices"], d["data"]


def _to_csc(m):
    """the CSC arrays of a CSR matrix (column entries by ascending row)"""
    shape, ip, ix, dt = m
    rows, cols = shape
    ip = np.asarray(ip, dtype=np.int64)
    ix = np.asarray(ix, dtype=np.int64)
    row_of = np.repeat(np.arange(rows), np.diff(ip))
    order = np.lexsort((row_of, ix))
    cip = np.zeros(cols + 1, dtype=np.int64)
    np.add.at(cip, ix + 1, 1)
    return tuple(shape), np.cumsum(cip), row_of[order], np.asarray(dt, dtype=np.float64)[order]


def _t(m):
    """the same arrays read in the other storage = the transpose"""
    shape, ip, ix, dt = m
    return (shape[1], shape[0]), ip, ix, dt


def _binop(a, b, op, stream=None):
    from sprs_amd import binop
    return binop.csmat_binop(a, b, op, stream=stream)


def _check(res, want, storage=0):
    got = res.to_host()
    assert res.storage() == storage
    assert same_mat(got, want), (got, want)
    assert int(got[1][0]) == 0 and int(got[1][-1]) == got[2].size == got[3].size     # a proper indptr, exact nnz


# ---- the reference's own tests (binop.rs:488-598) ----------------------------------------------------------------------------

GOLDEN = [("mat1_plus_mat2", ADD), ("mat1_minus_mat2", SUB), ("mat1_times_mat2", MUL)]


@pytest.mark.parametrize("idx,ptr", WIDTHS)
@pytest.mark.parametrize("storage", [0, 1])
def test_golden_mat1_mat2(golden, fx, storage, idx, ptr):
    """test_add1 / test_sub1 / test_mul1; the same arrays tagged CSC are the transposes, whose binop has the same arrays"""
    m1, m2 = as_csr(golden["mat1"]), as_csr(golden["mat2"])
    a, b = _mat(m1, storage, idx, ptr), _mat(m2, storage, idx, ptr)
    for name, op in GOLDEN:
        res = _binop(a, b, op)
        _check(res, as_csr(fx[name]), storage)
        assert res.index_bytes() == np.dtype(idx).itemsize and res.indptr_bytes() == np.dtype(ptr).itemsize
    _check(a + b, as_csr(fx["mat1_plus_mat2"]), storage)
    _check(a - b, as_csr(fx["mat1_minus_mat2"]), storage)
    from sprs_amd import binop
    _check(binop.mul_mat_same_storage(a, b), as_csr(fx["mat1_times_mat2"]), storage)


@pytest.mark.parametrize("idx,ptr", WIDTHS)
def test_golden_mixed_storage(golden, fx, idx, ptr):
    """csr + csc and csc - csr: rhs.to_other_storage() first, the result in lhs' storage (binop.rs:56-62, 103-109)"""
    m1, m2 = as_csr(golden["mat1"]), as_csr(golden["mat2"])
    _check(_mat(m1, 0, idx, ptr) + _mat(_to_csc(m2), 1, idx, ptr), as_csr(fx["mat1_plus_mat2"]), 0)
    _check(_mat(_to_csc(m1), 1, idx, ptr) - _mat(m2, 0, idx, ptr), _to_csc(as_csr(fx["mat1_minus_mat2"])), 1)


@pytest.mark.parametrize("idx,ptr", WIDTHS)
def test_golden_smul(golden, idx, ptr):
    """test_smul: &mat1() * 2. == mat1_times_2()"""
    a = _mat(as_csr(golden["mat1"]), 0, idx, ptr)
    _check(a * 2.0, as_csr(golden["mat1_times_2"]))
    _check(2.0 * a, as_csr(golden["mat1_times_2"]))
    _check(a * np.float64(2.0), as_csr(golden["mat1_times_2"]))


def test_golden_differing_row_patterns(fx):
    c = fx["differing_row_patterns"]
    _check(_mat(as_csr(c["a"])) + _mat(as_csr(c["b"])), as_csr(c["a_plus_b"]))


@pytest.mark.parametrize("dtype", [np.uint64, np.uint32, np.uint16])
def test_golden_csvec_binops(fx, dtype):
    c = fx["csvec_binops"]
    v1, v2, v3 = (_vec(_fxvec(c[k]), dtype) for k in ("vec1", "vec2", "vec3"))
    for res, want in ((v1 + v2, c["vec1_plus_vec2"]), (v1 + v3, c["vec1_plus_vec3"])):
        assert same_vec(res.to_host(), _fxvec(want))
        assert res.index_bytes() == np.dtype(dtype).itemsize


def test_golden_zero_sized_vector(fx):
    """zero_sized_vector_works_as_{left,right}_vector_operand: the dimension-0 operand takes the other's dimension"""
    c = fx["zero_sized_vector"]
    vector, zero = _vec(_fxvec(c["vector"])), _vec(_fxvec(c["zero"]))
    assert same_vec((vector + zero).to_host(), _fxvec(c["vector"]))
    assert same_vec((zero + vector).to_host(), _fxvec(c["vector"]))
    assert same_vec((zero + zero).to_host(), (0, [], []))


# ---- zeros, signed zeros, inf, NaN ---------------------------------------------------------------------------------------------

inf, nan = float("inf"), float("nan")
#        index: (lhs, rhs); None = not stored
ZERO_RULES = {
    0: (0.0, None), 1: (None, 0.0),            # an explicit zero on either side, alone
    2: (5.0, -5.0),                             # x + (-x)
    3: (0.0, 2.0), 4: (3.0, 0.0),               # an explicit zero beside a value
    5: (-0.0, None), 6: (None, -0.0),           # -0.0 alone on each side
    7: (inf, None), 8: (None, inf),             # inf * 0.0 = NaN: kept by mul
    9: (nan, None), 10: (None, nan),
    11: (-3.0, None),                           # -3 * 0 = -0.0: dropped in the matrix
    12: (-0.0, 0.0), 13: (0.0, -0.0), 14: (-0.0, -0.0),
    15: (1.5, 2.5), 16: (inf, -inf), 17: (4.0, 4.0),
    18: (2.0, -nan), 19: (None, -nan),          # x - NaN hands the NaN on with ITS sign (subsd / fsub), as x + NaN does
}


def _zero_rule_lists():
    li = [k for k, (l, r) in ZERO_RULES.items() if l is not None]
    ri = [k for k, (l, r) in ZERO_RULES.items() if r is not None]
    return li, [ZERO_RULES[k][0] for k in li], ri, [ZERO_RULES[k][1] for k in ri]


def test_zero_rules_matrix():
    li, lv, ri, rv = _zero_rule_lists()
    # two copies of the pattern and an empty slice between them
    a = ((3, 20), [0, len(li), len(li), 2 * len(li)], li + li, lv + lv)
    b = ((3, 20), [0, len(ri), len(ri), 2 * len(ri)], ri + ri, rv + rv)
    da, db = _mat(a), _mat(b)
    for op in OPS:
        want = csmat_binop_ref(a, b, op)
        _check(_binop(da, db, op), want)
        row0 = dict(zip(want[2][:want[1][1]].tolist(), want[3][:want[1][1]].tolist()))
        if op == ADD:
            assert not {0, 1, 2, 5, 6, 12, 13, 14} & set(row0) and row0[3] == 2.0 and np.isnan(row0[16]) and row0[17] == 8.0
        if op == SUB:
            assert not {0, 1, 5, 6, 12, 13, 14, 17} & set(row0) and row0[2] == 10.0 and row0[8] == -inf
        if op == MUL:
            assert sorted(row0) == [2, 7, 8, 9, 10, 15, 16, 17, 18, 19] and row0[2] == -25.0 and all(np.isnan(row0[k]) for k in (7, 8, 9, 10)) and row0[16] == -inf


def test_zero_rules_vector():
    """csvec_binop drops nothing: -0.0 + 0.0 = +0.0, 0.0 - (-0.0) = +0.0 and -0.0 - 0.0 = -0.0 are stored"""
    li, lv, ri, rv = _zero_rule_lists()
    v, w = (20, li, lv), (20, ri, rv)
    dv, dw = _vec(v), _vec(w)
    from sprs_amd import binop
    for op in OPS:
        want = csvec_binop_ref(v, w, op)
        assert want[1].tolist() == sorted(ZERO_RULES)
        assert same_vec(binop.csvec_binop(dv, dw, op).to_host(), want)
    add = dict(zip(*(x.tolist() for x in (dv + dw).to_host()[1:])))
    sub = dict(zip(*(x.tolist() for x in (dv - dw).to_host()[1:])))
    assert add[12] == 0.0 and not np.signbit(add[12])          # -0.0 + 0.0 = +0.0
    assert sub[13] == 0.0 and not np.signbit(sub[13])          # 0.0 - (-0.0) = +0.0
    assert sub[12] == 0.0 and np.signbit(sub[12])              # -0.0 - 0.0 = -0.0
    assert add[5] == 0.0 and not np.signbit(add[5]) and add[2] == 0.0
    assert np.isnan(sub[10]) and not np.signbit(sub[10]) and np.isnan(sub[18]) and np.signbit(sub[18]) and np.signbit(sub[19])


# ---- tile edges ----------------------------------------------------------------------------------------------------------------

def _rows_to_mat(rows, inner):
    """rows: list of (indices, values)"""
    ip = np.concatenate([[0], np.cumsum([len(r[0]) for r in rows])]).astype(np.int64)
    ix = np.concatenate([np.asarray(r[0], dtype=np.int64) for r in rows]) if rows else np.zeros(0, dtype=np.int64)
    dt = np.concatenate([np.asarray(r[1], dtype=np.float64) for r in rows]) if rows else np.zeros(0)
    return (len(rows), inner), ip, ix, dt


def _vals(n, seed):
    return np.random.default_rng(seed).integers(1, 9, n).astype(np.float64)    # exact sums, some equal pairs (a - b = 0)


EMPTY = ([], [])


def _slice_pair(n_both, n_l, n_r, seed, inner_off=0):
    """a slice pair with n_both shared indices, n_l lhs-only and n_r rhs-only ones, interleaved at random"""
    rng = np.random.default_rng(seed)
    kind = rng.permutation(np.concatenate([np.zeros(n_both, dtype=np.int64), np.ones(n_l, dtype=np.int64), np.full(n_r, 2)]))
    idx = np.arange(kind.size) * 2 + inner_off
    li, ri = idx[kind != 2], idx[kind != 1]
    return (li, _vals(li.size, seed + 1)), (ri, _vals(ri.size, seed + 2))


def _tile_cases(T, op):
    """name -> (a, b), one-slice cases first"""
    cases = {}
    full = np.arange(2 * T)
    cases["one_slice_all_pairs"] = (_rows_to_mat([(full, _vals(2 * T, 1))], 2 * T + 1), _rows_to_mat([(full, _vals(2 * T, 2))], 2 * T + 1))
    # one leading lhs-only entry shifts every pair by one slot: with the case above, both parities of a pair at a tile edge
    lead = np.concatenate([[0], full + 1])
    cases["one_slice_shifted_pairs"] = (_rows_to_mat([(lead, _vals(2 * T + 1, 3))], 2 * T + 1),
                                        _rows_to_mat([(full + 1, _vals(2 * T, 4))], 2 * T + 1))
    cases["lhs_empty"] = (_rows_to_mat([EMPTY], 2 * T + 1), _rows_to_mat([(full, _vals(2 * T, 5))], 2 * T + 1))
    cases["rhs_empty"] = (_rows_to_mat([(full, _vals(2 * T, 6))], 2 * T + 1), _rows_to_mat([EMPTY], 2 * T + 1))
    cases["both_empty"] = (_rows_to_mat([EMPTY], 7), _rows_to_mat([EMPTY], 7))
    # every slot cancels: whole tiles emit nothing
    x = _vals(2 * T, 7)
    other = {ADD: -x, SUB: x, MUL: np.zeros(2 * T)}[op]
    cases["all_cancel"] = (_rows_to_mat([(full, x)], 2 * T + 1), _rows_to_mat([(full, other)], 2 * T + 1))
    n_one = len(cases)
    # a slice of T slots, empty slices ON the tile edge, a slice of 3T + 1 slots, empty slices, a slice that ends on a tile
    # edge again, trailing empty slices
    inner = 8 * T
    l0, r0 = _slice_pair(T // 4, T // 4, T // 4, 11)                    # T slots
    l1, r1 = _slice_pair(T, T // 2, T // 2 + 1, 12)                     # 3T + 1 slots
    l2, r2 = _slice_pair(T // 2 - 1, 0, 1, 13)                          # T - 1 slots: ends at slot 5T
    l3, r3 = _slice_pair(3, 2, 2, 14)
    la = [l0] + [EMPTY] * 5 + [l1] + [EMPTY] * 3 + [l2] + [EMPTY] * 4
    lb = [r0] + [EMPTY] * 5 + [r1] + [EMPTY] * 3 + [r2] + [EMPTY] * 4
    cases["long_slice_between_empty_runs"] = (_rows_to_mat(la, inner), _rows_to_mat(lb, inner))
    cases["trailing_empty_off_edge"] = (_rows_to_mat(la + [l3] + [EMPTY] * 300, inner), _rows_to_mat(lb + [r3] + [EMPTY] * 300, inner))
    cases["cancel_then_more"] = (_rows_to_mat([EMPTY, (full, x), EMPTY, l3], 2 * T + 1), _rows_to_mat([EMPTY, (full, other), EMPTY, r3], 2 * T + 1))
    # more slices than slots in one tile (their starts no longer fit the tile's table): runs of empty slices around short ones
    many = 2 * T + 100
    cases["many_empty_slices"] = (_rows_to_mat([l3] + [EMPTY] * many + [l0, l3] + [EMPTY] * many + [l3, EMPTY], inner),
                                  _rows_to_mat([r3] + [EMPTY] * many + [r0, r3] + [EMPTY] * many + [r3, EMPTY], inner))
    cases["outer_zero"] = (_rows_to_mat([], 5), _rows_to_mat([], 5))
    return cases, n_one


@pytest.mark.parametrize("op", OPS)
def test_tile_edges(tile, op):
    cases, n_one = _tile_cases(tile, op)
    from sprs_amd import binop
    for pos, (name, (a, b)) in enumerate(cases.items()):
        want = csmat_binop_vec(a, b, op)
        assert same_mat(_binop(_mat(a), _mat(b), op).to_host(), want), name
        assert same_mat(_binop(_mat(_t(a), 1, np.uint32, np.uint32), _mat(_t(b), 1, np.uint32, np.uint32), op).to_host(), _t(want)), name
        if pos < n_one:
            v, w = (a[0][1], a[2], a[3]), (b[0][1], b[2], b[3])
            assert same_vec(binop.csvec_binop(_vec(v), _vec(w), op).to_host(), csvec_binop_vec(v, w, op)), name
    if op == ADD:
        assert csmat_binop_vec(*cases["all_cancel"], op)[2].size == 0
        want = csmat_binop_vec(*cases["long_slice_between_empty_runs"], op)
        s = cases["long_slice_between_empty_runs"][0][1] + cases["long_slice_between_empty_runs"][1][1]
        assert s[1] == tile and s[7] - s[6] == 3 * tile + 1 and s[-1] == 5 * tile and want[2].size > 2 * tile


# ---- ragged random matrices ----------------------------------------------------------------------------------------------------

def _ragged(seed, rows=600, cols=200):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 30, rows)
    lens[rng.choice(rows, 4, replace=False)] = rng.integers(150, cols, 4)
    m = ragged_csr(lens, cols, seed=seed, positive=False)
    dt = np.round(m[3] * 4) / 4                     # quarters: exact cancellations and explicit zeros do occur
    return m[0], m[1], m[2], dt


@pytest.fixture(scope="module")
def ragged_pair():
    a, b = _ragged(31), _ragged(32)
    assert a[2].size + b[2].size <= 20000
    return a, b, {op: csmat_binop_vec(a, b, op) for op in OPS}


@pytest.mark.parametrize("idx,ptr", IDX_COMBOS)
def test_ragged_random(ragged_pair, idx, ptr):
    a, b, want = ragged_pair
    da, db = _mat(a, 0, idx, ptr), _mat(b, 0, idx, ptr)
    for op in OPS:
        _check(_binop(da, db, op), want[op])
    assert want[MUL][2].size > 100 and want[ADD][2].size + want[MUL][2].size < a[2].size + b[2].size   # pairs, and dropped zeros
    # mixed storage: B given as CSC
    _check(da - _mat(_to_csc(b), 1, idx, ptr), want[SUB])


def test_hub_row_matches_the_csvec_path():
    """all entries in one slice: the same kernels as the vector path give the same bits"""
    from sprs_amd import binop
    rng = np.random.default_rng(5)
    n = 9000
    li, ri = np.sort(rng.choice(n, 3000, replace=False)), np.sort(rng.choice(n, 3500, replace=False))
    lv, rv = rng.standard_normal(3000), rng.standard_normal(3500)
    rows_a = [EMPTY] * 3 + [(li, lv)] + [EMPTY] * 3
    rows_b = [EMPTY] * 3 + [(ri, rv)] + [EMPTY] * 3
    da, db = _mat(_rows_to_mat(rows_a, n)), _mat(_rows_to_mat(rows_b, n))
    dv, dw = _vec((n, li, lv)), _vec((n, ri, rv))
    for op in OPS:
        _, mip, mix, mdt = _binop(da, db, op).to_host()
        _, vix, vdt = binop.csvec_binop(dv, dw, op).to_host()
        keep = ~(vdt == 0.0)                       # the matrix drops zeros (one-sided products), the vector keeps them
        assert np.array_equal(mix, vix[keep]) and np.array_equal(bits(mdt), bits(vdt[keep]))
        assert mip.tolist() == [0] * 4 + [mix.size] * 4
        assert same_vec((n, vix, vdt), csvec_binop_vec((n, li, lv), (n, ri, rv), op))


# ---- scale -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("storage", [0, 1])
def test_scale(storage):
    from sprs_amd.device import DeviceVec
    a = _ragged(41, rows=150, cols=200)
    a[3][::7] = 0.0                                # stored zeros
    a[3][3] = -0.0
    m = a if storage == 0 else _t(a)
    da = _mat(m, storage)
    x = np.random.default_rng(3).standard_normal(m[0][1])
    y0 = (da * DeviceVec.from_host(x)).to_host()
    for s in (2.0, -0.5, 0.0, -0.0, 1e-310, inf):
        res = da * s
        shape, ip, ix, dt = res.to_host()
        assert res.storage() == storage and tuple(shape) == tuple(m[0])
        assert np.array_equal(ip.astype(np.int64), a[1]) and np.array_equal(ix.astype(np.int64), a[2])   # nothing dropped
        with np.errstate(invalid="ignore"):
            assert np.array_equal(bits(dt), bits(a[3] * s))
    # one entry, and an even count: the 16-byte body and its tail
    for n in (1, 2, 5):
        one = ((1, 8), [0, n], list(range(n)), [3.0] * n)
        assert same_mat((_mat(one) * 0.5).to_host(), ((1, 8), [0, n], list(range(n)), [1.5] * n))
    # the operand is untouched and still multiplies
    assert same_mat(da.to_host(), m)
    assert np.array_equal(bits((da * DeviceVec.from_host(x)).to_host()), bits(y0))


def test_operands_unchanged_and_reusable(ragged_pair):
    from sprs_amd.device import DeviceVec
    a, b, want = ragged_pair
    da, db = _mat(a), _mat(b)
    x = np.random.default_rng(4).standard_normal(a[0][1])
    y0 = (da * DeviceVec.from_host(x)).to_host()       # builds a plan on the handle
    c = da + db
    assert same_mat(da.to_host(), a) and same_mat(db.to_host(), b)
    assert np.array_equal(bits((da * DeviceVec.from_host(x)).to_host()), bits(y0))
    # the result is an ordinary handle: I - 0.1 * C style chains
    _check(c - db, csmat_binop_vec(want[ADD], b, SUB))


# ---- errors ------------------------------------------------------------------------------------------------------------------

def test_errors(golden):
    from sprs_amd import SprsHipError, _ffi, binop
    m1 = as_csr(golden["mat1"])
    a = _mat(m1)
    small = _mat(((4, 5), m1[1][:5], m1[2][:int(m1[1][4])], m1[3][:int(m1[1][4])]))
    for f in (lambda: a + small, lambda: a - small, lambda: _binop(a, small, MUL), lambda: a + _mat(((5, 4), [0] * 5, [], []), 1)):
        with pytest.raises(SprsHipError) as e:
            f()
        assert e.value.status == _ffi.DIM_MISMATCH and str(e.value).endswith("Dimension mismatch")
    a_csc = _mat(m1, 1)
    for op in OPS:                                  # the strict entry: csmat_binop asserts equal storage
        with pytest.raises(SprsHipError) as e:
            _binop(a, a_csc, op)
        assert e.value.status == _ffi.STORAGE_MISMATCH and str(e.value).endswith("Storage mismatch")
    with pytest.raises(SprsHipError) as e:
        binop.mul_mat_same_storage(a_csc, a)
    assert e.value.status == _ffi.STORAGE_MISMATCH
    for other in (_mat(m1, 0, np.uint32, np.uint64), _mat(m1, 0, np.uint64, np.uint32), _mat(m1, 0, np.uint16, np.uint16)):
        for f in (lambda: a + other, lambda: other - a, lambda: _binop(a, other, MUL)):
            with pytest.raises(SprsHipError) as e:
                f()
            assert e.value.status == _ffi.STORAGE_MISMATCH
    with pytest.raises(SprsHipError) as e:
        _binop(a, a, 3)
    assert e.value.status == _ffi.INVALID_ARG
    v8, v9, z = _vec((8, [1], [1.0])), _vec((9, [1], [1.0])), _vec((0, [], []))
    for f in (lambda: v8 + v9, lambda: v9 - v8):
        with pytest.raises(SprsHipError) as e:
            f()
        assert e.value.status == _ffi.DIM_MISMATCH and str(e.value).endswith("Dimension mismatch")
    assert (z - v9).to_host()[0] == 9 and (v8 + z).to_host()[0] == 8          # fix_zeros comes first
    with pytest.raises(SprsHipError) as e:
        v8 + _vec((8, [1], [1.0]), np.uint32)
    assert e.value.status == _ffi.STORAGE_MISMATCH
    with pytest.raises(SprsHipError) as e:
        binop.csvec_binop(v8, v8, 7)
    assert e.value.status == _ffi.INVALID_ARG


def test_result_nnz_overflows_the_declared_indptr_type():
    """Iptr::from_usize(nnz) (binop.rs:268) panics when the result's nnz does not fit Iptr: 40000 + 40000 entries with u16"""
    from sprs_amd import SprsHipError, _ffi
    n = 40000
    a = ((2, n), np.array([0, n, n]), np.arange(n), np.ones(n))
    b = ((2, n), np.array([0, 0, n]), np.arange(n), np.ones(n))
    da, db = _mat(a, 0, np.uint16, np.uint16), _mat(b, 0, np.uint16, np.uint16)
    with pytest.raises(SprsHipError) as e:
        da + db
    assert e.value.status == _ffi.INDEX_OVERFLOW
    _check(_binop(da, da, SUB), ((2, n), [0, 0, 0], [], []))


def test_overflow_message_survives_the_converted_rhs():
    """the same sum with a CSC rhs: `&lhs + &rhs` converts it first (binop.rs:52-64), and releasing that temporary on the way
    out of the failed call must leave the status AND the message the CSR rhs gives"""
    from sprs_amd import SprsHipError, _ffi
    n = 40000
    a = ((2, n), np.array([0, n, n]), np.arange(n), np.ones(n))
    b = ((2, n), np.array([0, 0, n]), np.arange(n), np.ones(n))
    b_csc = ((2, n), np.arange(n + 1), np.ones(n, dtype=np.int64), np.ones(n))      # the same matrix by columns
    da = _mat(a, 0, np.uint16, np.uint16)
    seen = []
    for db in (_mat(b, 0, np.uint16, np.uint16), _mat(b_csc, 1, np.uint16, np.uint16)):
        with pytest.raises(SprsHipError) as e:
            da + db
        assert e.value.status == _ffi.INDEX_OVERFLOW
        seen.append(str(e.value))
    assert seen[0].endswith("nnz of the result (80000)")
    assert seen[1] == seen[0]


# ---- real device only -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def rmat_pair():
    import torch
    from sprs_amd import gen
    n = 200000
    out = []
    for seed in (3, 4):                             # (generated on the device: seconds on the host)
        ip, ix, dt = gen.rmat_csr(n, 8, seed=seed, value_seed=seed + 10, device=torch.device("cuda", 0))
        out.append(((n, n), ip.cpu().numpy().astype(np.int64), ix.cpu().numpy().astype(np.int64), dt.cpu().numpy()))
    return out


@pytest.mark.skipif(EMULATED, reason="large operands: real device only")
def test_rmat_200k(rmat_pair):
    a, b = rmat_pair
    da, db = _mat(a, 0, np.uint32, np.uint64), _mat(b, 0, np.uint32, np.uint64)
    _check(da + db, csmat_binop_vec(a, b, ADD))
    _check(da - db, csmat_binop_vec(a, b, SUB))
    _check(_binop(da, db, MUL), csmat_binop_vec(a, b, MUL))
    # A + A^T: the transpose view is the same arrays tagged CSC; the operator converts it
    at = _t(_to_csc(a))                              # A^T as CSR
    sym = da + da.transpose_view()
    _check(sym, csmat_binop_vec(a, at, ADD))
    got = sym.to_host()
    assert same_mat(_to_csc(got), got)               # symmetric structure and values (x + y == y + x bitwise)


@pytest.mark.skipif(EMULATED, reason="torch streams: real device only")
def test_non_blocking_stream(ragged_pair):
    """the operands are written on a non-blocking torch stream and added there with no host synchronise in between: the
    read-back of the result's nnz is ordered on that stream"""
    import torch
    from sprs_amd import binop
    from sprs_amd.device import DeviceCsMat
    a, b, want = ragged_pair
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        t = []
        for m in (a, b):
            ip = torch.zeros(m[1].size, dtype=torch.int64, device=dev)
            ix = torch.zeros(m[2].size, dtype=torch.int64, device=dev)
            dt = torch.zeros(m[3].size, dtype=torch.float64, device=dev)
            t.append((ip, ix, dt))
        torch.cuda._sleep(20_000_000)                  # keep the stream busy: the copies below land late
        for m, (ip, ix, dt) in zip((a, b), t):
            ip.copy_(torch.from_numpy(m[1]).to(dev, non_blocking=True))
            ix.copy_(torch.from_numpy(m[2]).to(dev, non_blocking=True))
            dt.copy_(torch.from_numpy(m[3]).to(dev, non_blocking=True))
        da, db = (DeviceCsMat.wrap_torch(m[0], *arrs) for m, arrs in zip((a, b), t))
        res = binop.csmat_binop(da, db, ADD, stream=s)
        scaled = binop.scale(da, 3.0, stream=s)
    _check(res, want[ADD])
    assert np.array_equal(bits(scaled.to_host()[3]), bits(a[3] * 3.0))
