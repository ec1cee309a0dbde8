"""Device matrix extraction (csmat.rs:1017-1056, 1219-1256, 1312-1351): outer_view, diag, the batched nnz_index / get and
to_inner_onehot against the plain-Python restatement (tests/extract_ref.py) — indptr, indices and value bits.

Sizes follow the kernels' constants (extract.hpp): groups of 64 outer slices per wave, workgroups of 256, EX_LONG = 128 entries from
which a slice is scanned by the whole wave, 64 entries per load and 8 loads (512 entries) per step.  The file also runs against the kernel emulator
(tests/test_extract_emu_cpu.py)."""
import json
import os

import numpy as np
import pytest

import extract_ref as ref
from helpers import fresh_blocks, ragged_csr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NAN = float("nan")
NONE = (1 << 64) - 1
EX_LONG = 128
CSR, CSC = 0, 1


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module", autouse=True)
def _need_device():
    import sprs_amd
    if sprs_amd.device_count() < 1:
        pytest.skip("no HIP device")


@pytest.fixture(scope="module")
def fx():
    return json.load(open(os.path.join(HERE, "golden", "reduce_fixtures.json")))


def _data(a):
    return np.array([NAN if x == "nan" else float(x) for x in a], dtype=np.float64)


def _mat(shape, ip, ix, dt, storage=CSR, idx=np.uint64, ptr=np.uint64):
    from sprs_amd.device import DeviceCsMat
    return DeviceCsMat.from_host(tuple(shape), np.asarray(ip, dtype=ptr), np.asarray(ix, dtype=idx), np.asarray(dt, dtype=np.float64),
                                 storage=storage)


def _fx_mat(m, **kw):
    return _mat(m["shape"], m["indptr"], m["indices"], _data(m["data"]), storage=CSC if m["storage"] == "csc" else CSR, **kw)


def _same_vec(res, dim, idx, val, dtype=None):
    d, i, v = res.to_host()
    assert d == dim and np.array_equal(i.astype(np.int64), np.asarray(idx, dtype=np.int64)), (d, i, idx)
    assert np.array_equal(bits(v), bits(val)), (v, val)
    if dtype is not None:
        assert i.dtype == dtype


def _random_slices(lens, inner, seed, drop_diag=(), zero_diag=()):
    """compressed arrays with the given slice lengths whose slice i holds inner index i unless i is in drop_diag; the diagonal
    value of the slices in zero_diag is an explicit 0.0"""
    rng = np.random.default_rng(seed)
    ip, ix, dt = [0], [], []
    for o, n in enumerate(lens):
        n = min(n, inner)
        c = set(rng.choice(inner, n, replace=False).tolist()) if n else set()
        if o < inner and n and o not in drop_diag:
            if o not in c:
                c.pop()
                c.add(o)
        else:
            c.discard(o)
        c = sorted(c)
        vals = rng.standard_normal(len(c))
        if o in zero_diag and o in c:
            vals[c.index(o)] = 0.0
        ix += c
        dt += vals.tolist()
        ip.append(len(ix))
    return np.array(ip), np.array(ix, dtype=np.int64), np.array(dt)


# ---- diag ----------------------------------------------------------------------------------------------------------------------------

def test_golden_diag(fx):
    """csmat.rs:2875-2948 diag and diag_rectangular"""
    for name in ("diag", "diag_rectangular"):
        e = fx[name]["expected"]
        d = _fx_mat(fx[name]).diag()
        _same_vec(d, e["dim"], e["indices"], e["data"])
        d.check_structure()


@pytest.mark.parametrize("storage", [CSR, CSC])
@pytest.mark.parametrize("outer", [63, 64, 65, 255, 256, 257])
def test_diag_outer_sizes(outer, storage):
    """both storages, rows > cols and rows < cols, empty slices, missing diagonal entries, an explicit zero kept"""
    rng = np.random.default_rng(outer)
    for inner in (outer + 9, max(outer - 9, 1)):
        lens = rng.integers(0, 12, outer)
        lens[rng.choice(outer, 6, replace=False)] = 0
        drop = set(rng.choice(outer, outer // 5, replace=False).tolist()) - {1}
        lens[1] = 5
        zero = {k for k in (1, 40, outer - 1) if k not in drop}
        ip, ix, dt = _random_slices(lens, inner, seed=outer + inner, drop_diag=drop, zero_diag=zero)
        shape = (outer, inner) if storage == CSR else (inner, outer)
        fresh_blocks()
        d = _mat(shape, ip, ix, dt, storage=storage).diag()
        n, ei, ed = ref.diag(shape, ip, ix, dt)
        assert n == min(shape) and 0 < ei.size < n
        _same_vec(d, n, ei, ed)
        kept_zero = [k for k in zero if k < n and lens[k] > 0]
        assert kept_zero and all(k in ei.tolist() for k in kept_zero) and 0.0 in ed.tolist()
        d.check_structure()


@pytest.mark.parametrize("where", ["first", "last", "absent"])
def test_diag_in_a_long_slice(where):
    """a slice of 64 * 3 + 1 entries with the diagonal as its first entry, its last entry, or not stored"""
    n_outer, inner, long_len = 250, 500, 64 * 3 + 1
    o = {"first": 0, "last": 200, "absent": 30}[where]
    cols = {"first": np.arange(long_len), "last": np.arange(o - long_len + 1, o + 1),
            "absent": np.concatenate([np.arange(o), np.arange(o + 1, long_len + 1)])}[where]
    assert cols.size == long_len and (cols[0] == o if where == "first" else cols[-1] == o if where == "last" else o not in cols)
    ip, ix, dt = _random_slices([2] * n_outer, inner, seed=3)
    s, e = int(ip[o]), int(ip[o + 1])
    ix = np.concatenate([ix[:s], cols, ix[e:]])
    dt = np.concatenate([dt[:s], np.random.default_rng(4).standard_normal(long_len), dt[e:]])
    ip = ip.copy()
    ip[o + 1:] += long_len - (e - s)
    shape = (n_outer, inner)
    res = _mat(shape, ip, ix, dt).diag()
    dim, ei, ed = ref.diag(shape, ip, ix, dt)
    assert (o in ei.tolist()) == (where != "absent")
    _same_vec(res, dim, ei, ed)


@pytest.mark.parametrize("idx,ptr", [(np.uint64, np.uint64), (np.uint32, np.uint32), (np.uint32, np.uint64), (np.uint64, np.uint32),
                                     (np.uint16, np.uint16)])
def test_diag_index_widths(idx, ptr):
    """4- and 8-byte indices and declared 2: the result has the matrix's index type"""
    lens = np.full(100, 3)
    ip, ix, dt = _random_slices(lens, 120, seed=7, drop_diag={5, 64, 99})
    res = _mat((100, 120), ip, ix, dt, idx=idx, ptr=ptr).diag()
    dim, ei, ed = ref.diag((100, 120), ip, ix, dt)
    _same_vec(res, dim, ei, ed, dtype=idx)
    res.check_structure()


def test_diag_of_an_empty_matrix():
    _same_vec(_mat((5, 7), np.zeros(6), [], []).diag(), 5, [], [])
    _same_vec(_mat((0, 7), np.zeros(1), [], []).diag(), 0, [], [])
    _same_vec(_mat((3, 3), [0, 1, 1, 2], [1, 0], [1.0, 2.0]).diag(), 3, [], [])


# ---- outer_view ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("storage", [CSR, CSC])
@pytest.mark.parametrize("idx,ptr", [(np.uint64, np.uint64), (np.uint32, np.uint32), (np.uint16, np.uint32)])
def test_outer_view_every_slice(idx, ptr, storage):
    """every slice of a small ragged matrix equals the host slice (an empty one included); i = outer gives None"""
    lens = [3, 0, 7, 1, 0, 0, 12, 5, 64, 2, 65]
    shape, ip, ix, dt = ragged_csr(lens, 90, seed=2, positive=False)
    if storage == CSC:
        shape = (shape[1], shape[0])
    m = _mat(shape, ip, ix, dt, storage=storage, idx=idx, ptr=ptr)
    for i in range(len(lens)):
        vi, vd = ref.outer_view(ip, ix, dt, i)
        v = m.outer_view(i)
        assert v.dim() == 90 and v.nnz() == lens[i] and v.index_bytes() == np.dtype(idx).itemsize
        _same_vec(v, 90, vi, vd, dtype=idx)
    assert m.outer_view(len(lens)) is None and m.outer_view(len(lens) + 5) is None


def test_outer_view_keeps_the_matrix_alive():
    """the view borrows the matrix's arrays: it still reads correctly after the Python name of the matrix is dropped"""
    import gc
    shape, ip, ix, dt = ragged_csr([4, 9, 130, 2], 400, seed=6, positive=False)
    m = _mat(shape, ip, ix, dt)
    v = m.outer_view(2)
    del m
    gc.collect()
    fresh_blocks()
    junk = [_mat(shape, ip, ix, np.full(dt.size, 7.0)) for _ in range(4)]      # would recycle the blocks of a freed matrix
    vi, vd = ref.outer_view(ip, ix, dt, 2)
    _same_vec(v, 400, vi, vd)
    assert len(junk) == 4


def test_outer_view_as_an_operand():
    """the view is usable as an operand of dot and as the rhs of lsolve_csc_sparse_rhs"""
    import reduce_ref
    from sprs_amd import linalg
    from sprs_amd.device import DeviceCsVec
    # a lower triangular CSC matrix: column j holds rows j (the pivot), j + 2, j + 5
    n = 40
    ip, ix, dt = [0], [], []
    rng = np.random.default_rng(12)
    for j in range(n):
        r = [k for k in (j, j + 2, j + 5) if k < n]
        ix += r
        dt += [2.0] + rng.integers(1, 4, len(r) - 1).astype(float).tolist()
        ip.append(len(ix))
    ip, ix, dt = np.array(ip), np.array(ix), np.array(dt)
    l = _mat((n, n), ip, ix, dt, storage=CSC)
    col = l.outer_view(30)
    vi, vd = ref.outer_view(ip, ix, dt, 30)
    other = DeviceCsVec.from_host(n, np.array([3, 32, 35], dtype=np.uint64), np.array([5.0, 7.0, 11.0]))
    assert col.dot(other) == reduce_ref.dot_merge(vi, vd, [3, 32, 35], [5.0, 7.0, 11.0]) != 0.0
    assert col.dot(col) == reduce_ref.squared_l2_norm(vd) == col.squared_l2_norm()
    x = linalg.lsolve_csc_sparse_rhs(l, col)
    owned = DeviceCsVec.from_host(n, vi.astype(np.uint64), vd)
    want = linalg.lsolve_csc_sparse_rhs(l, owned)
    d, xi, xv = x.to_host()
    wd, wi, wv = want.to_host()
    assert d == wd == n and np.array_equal(xi, wi) and np.array_equal(bits(xv), bits(wv))
    # L x = column 30 of L has the solution e_30
    assert xi.tolist() == [30, 32, 34, 35, 36, 37, 38, 39][:len(xi)] or 30 in xi.tolist()
    assert xv[xi.tolist().index(30)] == 1.0 and np.all(xv[np.asarray(xi) != 30] == 0.0)


# ---- batched nnz_index / get ---------------------------------------------------------------------------------------------------------

def test_golden_nnz_index(fx):
    """csmat.rs:2622-2637 on CsMat::eye(11)"""
    from sprs_amd.device import DeviceCsMat
    q = fx["mat_nnz_index"]
    m = DeviceCsMat.eye(q["eye"])
    for row, col, want in q["queries"]:
        assert m.nnz_index(row, col) == want and m.nnz_index_outer_inner(row, col) == want
        assert m.get(row, col) == (None if want is None else 1.0) and m.get_outer_inner(row, col) == (None if want is None else 1.0)
    rows, cols = np.array([r for r, _, _ in q["queries"]]), np.array([c for _, c, _ in q["queries"]])
    assert m.nnz_index(rows, cols).tolist() == [NONE if w is None else w for _, _, w in q["queries"]]


@pytest.mark.parametrize("idx,ptr", [(np.uint64, np.uint64), (np.uint32, np.uint32)])
def test_batched_matrix_lookup_csr_and_csc(idx, ptr):
    """CSR and CSC give the same answers for the same (row, col); out-of-range rows and cols are None; pos indexes the
    downloaded data"""
    rows, cols = 37, 53
    shape, ip, ix, dt = ragged_csr(np.random.default_rng(3).integers(0, 20, rows), cols, seed=4, positive=False)
    a = _mat(shape, ip, ix, dt, idx=idx, ptr=ptr)
    c = a.to_other_storage()
    assert c.is_csc()
    rng = np.random.default_rng(5)
    qr = np.concatenate([rng.integers(0, rows, 300), [rows, rows + 7, 0, 1 << 40, 5]])
    qc = np.concatenate([rng.integers(0, cols, 300), [0, 3, cols, 2, 1 << 40]])
    want = [ref.nnz_index(ip, ix, False, int(r), int(k)) for r, k in zip(qr, qc)]
    assert None in want[:300] and any(w is not None for w in want[:300]) and want[300:] == [None] * 5
    pos = a.nnz_index(qr, qc)
    assert pos.tolist() == [NONE if w is None else w for w in want]
    val, found = a.get(qr, qc)
    assert found.tolist() == [w is not None for w in want]
    assert np.array_equal(bits(val), bits([0.0 if w is None else dt[w] for w in want]))
    _, cip, cix, cdt = c.to_host()
    cpos = c.nnz_index(qr, qc)
    cval, cfound = c.get(qr, qc)
    assert cfound.tolist() == found.tolist() and np.array_equal(bits(cval), bits(val))
    hit = cpos != np.uint64(NONE)
    assert np.array_equal(bits(cdt[cpos[hit].astype(np.int64)]), bits(val[hit]))          # pos indexes the downloaded data
    assert np.array_equal(cix[cpos[hit].astype(np.int64)].astype(np.int64), qr[hit])      # CSC: the inner index is the row
    assert [ref.nnz_index(cip, cix, True, int(r), int(k)) for r, k in zip(qr, qc)] == [None if p == NONE else p for p in cpos.tolist()]
    assert a.nnz_index_outer_inner(qr[:50], qc[:50]).tolist() == pos[:50].tolist()
    assert c.nnz_index_outer_inner(qc[:50], qr[:50]).tolist() == cpos[:50].tolist()
    assert a.nnz_index(np.zeros(0), np.zeros(0)).shape == (0,)


# ---- to_inner_onehot -----------------------------------------------------------------------------------------------------------------

def _check_onehot(shape, ip, ix, dt, storage=CSR, idx=np.uint64, ptr=np.uint64):
    fresh_blocks()
    res = _mat(shape, ip, ix, dt, storage=storage, idx=idx, ptr=ptr).to_inner_onehot()
    eip, eix, edt = ref.to_inner_onehot(ip, ix, dt)
    rshape, rip, rix, rdt = res.to_host()
    assert tuple(rshape) == tuple(shape) and res.storage() == storage
    assert rip.dtype == ptr and rix.dtype == idx
    assert np.array_equal(rip.astype(np.int64), eip), (rip, eip)
    assert np.array_equal(rix.astype(np.int64), eix), (rix, eix)
    assert np.array_equal(bits(rdt), bits(edt))
    res.check_structure()
    return eip, eix


def test_golden_onehot(fx):
    """csmat.rs:2951-2999 onehot_zero, onehot_eye, onehot_sparse_csc, onehot_ignores_nan"""
    assert len(fx["onehot"]) == 4
    for m in fx["onehot"]:
        res = _fx_mat(m).to_inner_onehot()
        e = m["expected"]
        shape, ip, ix, dt = res.to_host()
        assert list(shape) == m["shape"] and res.is_csc() == (m["storage"] == "csc"), m["name"]
        assert ip.tolist() == e["indptr"] and ix.tolist() == e["indices"] and dt.tolist() == e["data"], m["name"]


def test_onehot_ties_zeros_nans_infinities():
    inf = np.inf
    slices = [([2, 5, 7], [3.0, 3.0, 3.0]),        # first / middle / last equal: the last
              ([2, 5, 7], [3.0, 1.0, 3.0]),
              ([2, 5, 7], [3.0, 3.0, 1.0]),
              ([1, 4], [0.0, -0.0]),               # -0.0 == +0.0: the later one
              ([1, 4], [-0.0, 0.0]),
              ([1, 4], [NAN, NAN]),                # all NaN: unpopulated
              ([], []),
              ([0, 3, 6], [-inf, -inf, NAN]),      # -inf only
              ([0, 3], [inf, 1e308]),
              ([0, 8], [NAN, -5.0])]
    ip, ix, dt = [0], [], []
    for i, d in slices:
        ix += i
        dt += d
        ip.append(len(ix))
    eip, eix = _check_onehot((len(slices), 9), ip, ix, dt)
    assert eix.tolist() == [7, 7, 5, 4, 4, 3, 0, 8] and eip.tolist() == [0, 1, 2, 3, 4, 5, 5, 5, 6, 7, 8]


def test_onehot_empty_matrices():
    _check_onehot((3, 3), np.zeros(4), [], [])
    _check_onehot((0, 5), np.zeros(1), [], [])
    _check_onehot((4, 0), np.zeros(5), [], [])
    _check_onehot((2, 3), [0, 2, 3], [0, 2, 1], [NAN, NAN, NAN])          # entries, but no slice populated


@pytest.mark.parametrize("storage", [CSR, CSC])
@pytest.mark.parametrize("outer", [63, 64, 65])
def test_onehot_outer_sizes(outer, storage):
    rng = np.random.default_rng(outer)
    lens = rng.integers(0, 9, outer)
    shape, ip, ix, dt = ragged_csr(lens, 50, seed=outer, positive=False)
    dt = np.round(dt * 2) / 2                                              # coarse values: plenty of ties
    dt[rng.choice(dt.size, dt.size // 6, replace=False)] = NAN
    if storage == CSC:
        shape = (shape[1], shape[0])
    eip, _ = _check_onehot(shape, ip, ix, dt, storage=storage)
    assert 0 < eip[-1] < outer


@pytest.mark.parametrize("case", ["max_first", "max_last", "tie_across_chunks", "tie_first_last", "nan_tail"])
@pytest.mark.parametrize("length", [EX_LONG, EX_LONG + 1, 64 * 3 + 1, 512, 513, 1100])
def test_onehot_long_slices(length, case):
    """slices at and past the per-lane limit, longer than one load of 64 entries and than one wave step of 512, among short ones"""
    rng = np.random.default_rng(length)
    lens = [3, length, 0, 5, length, 2]
    shape, ip, ix, dt = ragged_csr(lens, 3000, seed=length, positive=False)
    for s in (ip[1], ip[4]):
        s = int(s)
        seg = rng.uniform(-1.0, 1.0, length)
        if case == "max_first":
            seg[0] = 5.0
        elif case == "max_last":
            seg[-1] = 5.0
        elif case == "tie_across_chunks":
            seg[63] = seg[64] = 5.0
            if length > 130:
                seg[127] = seg[130] = 5.0
        elif case == "tie_first_last":
            seg[0] = seg[-1] = 5.0
        else:
            seg[10] = 5.0
            seg[11:] = NAN
        dt[s:s + length] = seg
    eip, eix = _check_onehot(shape, ip, ix, dt)
    want_at = {"max_first": 0, "max_last": length - 1, "tie_across_chunks": 130 if length > 130 else 64, "tie_first_last": length - 1,
               "nan_tail": 10}[case]
    assert eix[1] == ix[int(ip[1]) + want_at] and eix[3] == ix[int(ip[4]) + want_at]


@pytest.mark.parametrize("idx,ptr", [(np.uint32, np.uint32), (np.uint32, np.uint64), (np.uint64, np.uint32), (np.uint16, np.uint16)])
def test_onehot_index_widths(idx, ptr):
    lens = [4, 0, 200, 7, 1]
    shape, ip, ix, dt = ragged_csr(lens, 250, seed=9, positive=False)
    _check_onehot(shape, ip, ix, dt, idx=idx, ptr=ptr)
