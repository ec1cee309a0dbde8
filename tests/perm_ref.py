"""CPU restatement of sprs/src/sparse/permutation.rs for the tests: the one loop all four matrix functions share
(permutation.rs:296-581), line by line, and a numpy twin for larger inputs.  A matrix is (shape, indptr, indices, data) with a
storage tag (0 CSR, 1 CSC); a permutation is a list / array `perm`, or None for the Identity variant."""
import numpy as np

CSR, CSC = 0, 1


def perm_is_valid(perm):
    """permutation.rs:39-49"""
    n = len(perm)
    seen = [False] * n
    for v in perm:
        v = int(v)
        if v < 0 or v >= n or seen[v]:
            return False
        seen[v] = True
    return True


def perm_new(perm):
    """PermOwned::new (permutation.rs:52-66) -> (perm, perm_inv)"""
    assert perm_is_valid(perm), "invalid permutation"
    perm = [int(v) for v in perm]
    inv = [0] * len(perm)
    for i, v in enumerate(perm):
        inv[v] = i
    return perm, inv


def _pair(perm):
    """perm_new, vectorised for the large permutations of the GPU tests"""
    if len(perm) < 1000:
        return perm_new(perm)
    perm = np.asarray(perm).astype(np.int64)
    n = perm.size
    assert perm.min() >= 0 and perm.max() < n and np.all(np.bincount(perm, minlength=n) == 1), "invalid permutation"
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    return perm, inv


def perm_mul(perm, x):
    """`&P * x` (permutation.rs:255-278); perm None = Identity"""
    if perm is None:
        return list(x)
    assert len(x) == len(perm), "Dimension mismatch"
    return [x[int(i)] for i in perm]


def is_identity(perm):
    """permutation.rs:144-152: elementwise"""
    if perm is not None and len(perm) >= 1000:
        return bool(np.array_equal(np.asarray(perm).astype(np.int64), np.arange(len(perm))))
    return perm is None or all(int(v) == i for i, v in enumerate(perm))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_mat(got, want):
    """shape, indptr, indices equal and the value BITS equal"""
    return (tuple(int(v) for v in got[0]) == tuple(int(v) for v in want[0])
            and np.array_equal(np.asarray(got[1]).astype(np.int64), np.asarray(want[1]).astype(np.int64))
            and np.array_equal(np.asarray(got[2]).astype(np.int64), np.asarray(want[2]).astype(np.int64))
            and np.array_equal(bits(got[3]), bits(want[3])))


def _copy(m):
    return m[0], np.array(m[1], dtype=np.int64), np.array(m[2], dtype=np.int64), np.array(m[3], dtype=np.float64)


def _apply_ref(m, o, g):
    """the loop of permutation.rs:322-339 / 377-394 / 465-481 / 555-571: for in_outer in o: the slice relabelled through g,
    stably sorted by the new index"""
    shape, ip, ix, dt = m
    ip = [int(v) for v in ip]
    outer = len(ip) - 1
    indptr, indices, data = [0], [], []
    for in_outer in (range(outer) if o is None else o):
        in_outer = int(in_outer)
        tmp = [((int(ix[k]) if g is None else g[int(ix[k])]), dt[k]) for k in range(ip[in_outer], ip[in_outer + 1])]
        tmp = sorted(tmp, key=lambda t: t[0])
        indptr.append(indptr[-1] + len(tmp))
        for ind, val in tmp:
            indices.append(ind)
            data.append(val)
    return shape, np.array(indptr, dtype=np.int64), np.array(indices, dtype=np.int64), np.array(data, dtype=np.float64)


def _apply_vec(m, o, g):
    """numpy twin: gather the slices, relabel, lexsort on (new outer, new inner)"""
    shape, ip, ix, dt = m
    ip = np.asarray(ip).astype(np.int64)
    ix = np.asarray(ix).astype(np.int64)
    dt = np.asarray(dt, dtype=np.float64)
    outer = ip.size - 1
    o = np.arange(outer) if o is None else np.asarray(o, dtype=np.int64)
    lens = (ip[1:] - ip[:-1])[o]
    indptr = np.zeros(outer + 1, dtype=np.int64)
    np.cumsum(lens, out=indptr[1:])
    new_outer = np.repeat(np.arange(outer), lens)
    src = np.repeat(ip[o] - indptr[:-1], lens) + np.arange(indptr[-1])
    new_inner = ix[src] if g is None else np.asarray(g, dtype=np.int64)[ix[src]]
    order = np.lexsort((new_inner, new_outer))
    return shape, indptr, new_inner[order], dt[src][order]


def _maps(m, storage, row_perm, col_perm):
    """(o, g) of the mapping table: CSR (p, q_), CSC (q, p_) (permutation.rs:544-547); None = identity on that side"""
    p = None if row_perm is None else _pair(row_perm)
    q = None if col_perm is None else _pair(col_perm)
    if storage == CSR:
        return (None if p is None else p[0]), (None if q is None else q[1])
    return (None if q is None else q[0]), (None if p is None else p[1])


def _paq(m, storage, row_perm, col_perm, apply):
    rows, cols = m[0]
    assert row_perm is None or len(row_perm) == rows, "Dimension mismatch"
    assert col_perm is None or len(col_perm) == cols, "Dimension mismatch"
    if (row_perm is None and col_perm is None) or rows == 0 or cols == 0:
        return _copy(m)
    o, g = _maps(m, storage, row_perm, col_perm)
    return apply(m, o, g)


def _papt(m, storage, perm, apply):
    rows, cols = m[0]
    assert rows == cols, "Dimension mismatch"
    assert perm is None or rows == len(perm), "Dimension mismatch"
    if is_identity(perm) or rows == 0:
        return _copy(m)
    p, p_ = _pair(perm)
    return apply(m, p, p_)                          # the same for CSR and CSC (permutation.rs:453-454)


def transform_mat_paq_ref(m, storage, row_perm, col_perm): return _paq(m, storage, row_perm, col_perm, _apply_ref)
def transform_mat_paq_vec(m, storage, row_perm, col_perm): return _paq(m, storage, row_perm, col_perm, _apply_vec)
def permute_rows_ref(m, storage, perm): return _paq(m, storage, perm, None, _apply_ref)
def permute_rows_vec(m, storage, perm): return _paq(m, storage, perm, None, _apply_vec)
def permute_cols_ref(m, storage, perm): return _paq(m, storage, None, perm, _apply_ref)
def permute_cols_vec(m, storage, perm): return _paq(m, storage, None, perm, _apply_vec)
def transform_mat_papt_ref(m, storage, perm): return _papt(m, storage, perm, _apply_ref)
def transform_mat_papt_vec(m, storage, perm): return _papt(m, storage, perm, _apply_vec)


def to_other(m, storage):
    """(shape, indptr, indices, data) of storage `storage` -> the same matrix in the other storage"""
    shape, ip, ix, dt = m
    ip = np.asarray(ip).astype(np.int64)
    ix = np.asarray(ix).astype(np.int64)
    dt = np.asarray(dt, dtype=np.float64)
    outer = ip.size - 1
    inner = shape[1] if storage == CSR else shape[0]
    outer_of = np.repeat(np.arange(outer), np.diff(ip))
    order = np.lexsort((outer_of, ix))
    nip = np.zeros(inner + 1, dtype=np.int64)
    np.add.at(nip, ix + 1, 1)
    return shape, np.cumsum(nip), outer_of[order], dt[order]


def transpose(m):
    """the same arrays read in the other storage = the transpose"""
    return (m[0][1], m[0][0]), m[1], m[2], m[3]
