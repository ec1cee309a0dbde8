"""CPU restatement of sprs/src/sparse/construct.rs and sprs/src/sparse/kronecker.rs for the tests: the five functions line by
line (with the append_outer_csvec and to_csr / to_csc calls inside them), and numpy twins for larger inputs.  A matrix is
(storage, shape, indptr, indices, data) with storage 0 = CSR, 1 = CSC; indptr may have a non-zero base (a slice view).  Where
the reference asserts, these raise AssertionError with its text."""
import numpy as np

CSR, CSC = 0, 1


def mat(storage, shape, indptr, indices, data):
    return (storage, (int(shape[0]), int(shape[1])), np.array(indptr, dtype=np.int64), np.array(indices, dtype=np.int64),
            np.array(data, dtype=np.float64))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_mat(got, want):
    """storage, shape, indptr, indices equal and the value BITS equal"""
    return (got[0] == want[0] and tuple(int(v) for v in got[1]) == tuple(int(v) for v in want[1])
            and np.array_equal(np.asarray(got[2]).astype(np.int64), np.asarray(want[2]).astype(np.int64))
            and np.array_equal(np.asarray(got[3]).astype(np.int64), np.asarray(want[3]).astype(np.int64))
            and np.array_equal(bits(got[4]), bits(want[4])))


def outer_dims(m): return m[1][0] if m[0] == CSR else m[1][1]
def inner_dims(m): return m[1][1] if m[0] == CSR else m[1][0]
def nnz(m): return int(m[2][-1]) - int(m[2][0])
def rows(m): return m[1][0]
def cols(m): return m[1][1]


def transpose(m):
    """transpose_view / transpose_mut (csmat.rs:982-991): the same arrays under the other tag"""
    return (1 - m[0], (m[1][1], m[1][0]), m[2], m[3], m[4])


def outer_iterator(m):
    """the outer slices as lists of (inner index, value) in stored order"""
    ip, base = m[2], int(m[2][0])
    for o in range(outer_dims(m)):
        s, e = int(ip[o]) - base, int(ip[o + 1]) - base
        yield [(int(m[3][k]), m[4][k]) for k in range(s, e)]


def _shape_of(storage, outer, inner):
    return (outer, inner) if storage == CSR else (inner, outer)


# ---- csmat.rs ------------------------------------------------------------------------------------------------------------------

def to_other_storage(m):
    """csmat.rs:1405-1426 over raw::convert_mat_storage (csmat.rs:1782-1829): histogram, cumulated sum, ordered fill"""
    inner = inner_dims(m)
    indptr = [0] * (inner + 1)
    indices = [0] * nnz(m)
    data = [0.0] * nnz(m)
    for vec in outer_iterator(m):
        for inner_dim, _ in vec:
            indptr[inner_dim] += 1
    cumsum = 0
    for i in range(len(indptr)):
        indptr[i], cumsum = cumsum, cumsum + indptr[i]
    assert indptr[-1] == nnz(m)
    for outer_dim, vec in enumerate(outer_iterator(m)):
        for inner_dim, val in vec:
            dest = indptr[inner_dim]
            data[dest] = val
            indices[dest] = outer_dim
            indptr[inner_dim] += 1
    last = 0
    for i in range(len(indptr)):
        indptr[i], last = last, indptr[i]
    return mat(1 - m[0], m[1], indptr, indices, data)


def to_owned(m):
    base = int(m[2][0])
    return mat(m[0], m[1], [int(v) - base for v in m[2]], m[3][:nnz(m)], m[4][:nnz(m)])


def to_csr(m): return to_owned(m) if m[0] == CSR else to_other_storage(m)      # csmat.rs:1438-1449
def to_csc(m): return to_owned(m) if m[0] == CSC else to_other_storage(m)      # csmat.rs:1451-1462


def zero(shape):
    """CsMatI::zero (csmat.rs:429-436): CSR, no entries"""
    return mat(CSR, shape, [0] * (shape[0] + 1), [], [])


def eye(dim):
    return mat(CSR, (dim, dim), list(range(dim + 1)), list(range(dim)), [1.0] * dim)


# ---- construct.rs --------------------------------------------------------------------------------------------------------------

def same_storage_fast_stack(mats):
    """construct.rs:10-45"""
    mats = list(mats)
    assert len(mats) != 0, "Empty stacking list"
    inner_dim = inner_dims(mats[0])
    assert all(inner_dims(x) == inner_dim for x in mats), "Dimension mismatch"
    storage_type = mats[0][0]
    assert all(x[0] == storage_type for x in mats), "Storage mismatch"
    indptr, indices, data = [0], [], []             # CsMatI::empty(storage_type, inner_dim)
    outer = 0
    for m in mats:
        for vec in outer_iterator(m):
            # res = res.append_outer_csvec(vec.view())  (csmat.rs:627-638): assert_eq!(self.inner_dims(), vec.dim()), the
            # slice's (index, value) pairs appended, one more indptr entry
            for i, val in vec:
                indices.append(i)
                data.append(val)
            indptr.append(len(indices))
            outer += 1
    return mat(storage_type, _shape_of(storage_type, outer, inner_dim), indptr, indices, data)


def vstack(mats):
    """construct.rs:48-63"""
    mats = list(mats)
    if all(m[0] == CSR for m in mats):
        return same_storage_fast_stack(mats)
    return same_storage_fast_stack([to_csr(m) for m in mats])


def hstack(mats):
    """construct.rs:66-81"""
    mats = list(mats)
    if all(m[0] == CSC for m in mats):
        return same_storage_fast_stack(mats)
    return same_storage_fast_stack([to_csc(m) for m in mats])


def bmat(mats):
    """construct.rs:94-160; a list of lists with None"""
    mats = [list(r) for r in mats]
    super_rows = len(mats)
    assert super_rows != 0, "Empty stacking list"
    super_cols = len(mats[0])
    assert super_cols != 0, "Empty stacking list"
    assert all(len(x) == super_cols for x in mats), "Dimension mismatch"
    assert not any(all(m is None for m in x) for x in mats), "Empty bmat row"
    assert not any(all(x[j] is None for x in mats) for j in range(super_cols)), "Empty bmat col"
    rows_per_row = [max([0] + [rows(m) for m in row if m is not None]) for row in mats]
    cols_per_col = [max([0] + [cols(row[j]) for row in mats if row[j] is not None]) for j in range(super_cols)]
    to_vstack = []
    for i, row in enumerate(mats):
        with_zeros = [zero((rows_per_row[i], cols_per_col[j])) if m is None else to_owned(m) for j, m in enumerate(row)]
        to_vstack.append(hstack(with_zeros))
    return vstack(to_vstack)


# ---- kronecker.rs --------------------------------------------------------------------------------------------------------------

def kronecker_product(a, b):
    """kronecker.rs:50-99.  a.kron(b) of two f64 is `self * b`: one multiply"""
    if a[0] == b[0]:
        was_csc = a[0] == CSC
        if was_csc:
            a, b = transpose(a), transpose(b)
        b_shape = b[1]
        shape = (a[1][0] * b[1][0], a[1][1] * b[1][1])
        values, indices, indptr = [], [], [0]
        element_count = 0
        b_slices = list(outer_iterator(b))
        with np.errstate(invalid="ignore", over="ignore"):
            for avec in outer_iterator(a):
                for bvec in b_slices:
                    for ai, av in avec:
                        for bi, bv in bvec:
                            indices.append(ai * b_shape[1] + bi)
                            element_count += 1
                            values.append(np.float64(av) * np.float64(bv))
                    indptr.append(element_count)
        res = mat(CSR, shape, indptr, indices, values)
        return transpose(res) if was_csc else res
    return kronecker_product(a, to_other_storage(to_owned(b)))


# ---- numpy twins ---------------------------------------------------------------------------------------------------------------

def to_other_storage_vec(m):
    m = to_owned(m)
    ip, ix, dt = m[2], m[3], m[4]
    outer_of = np.repeat(np.arange(ip.size - 1), np.diff(ip))
    order = np.lexsort((outer_of, ix))
    nip = np.zeros(inner_dims(m) + 1, dtype=np.int64)
    np.add.at(nip, ix + 1, 1)
    return (1 - m[0], m[1], np.cumsum(nip), outer_of[order], dt[order])


def same_storage_fast_stack_vec(mats):
    mats = [to_owned(m) for m in mats]
    assert len(mats) != 0, "Empty stacking list"
    assert all(inner_dims(x) == inner_dims(mats[0]) for x in mats), "Dimension mismatch"
    assert all(x[0] == mats[0][0] for x in mats), "Storage mismatch"
    shift = np.cumsum([0] + [nnz(m) for m in mats])
    indptr = np.concatenate([[0]] + [m[2][1:] + shift[k] for k, m in enumerate(mats)]).astype(np.int64)
    outer = sum(outer_dims(m) for m in mats)
    return (mats[0][0], _shape_of(mats[0][0], outer, inner_dims(mats[0])), indptr, np.concatenate([m[3] for m in mats]).astype(np.int64),
            np.concatenate([m[4] for m in mats]).astype(np.float64))


def vstack_vec(mats):
    return same_storage_fast_stack_vec([m if m[0] == CSR else to_other_storage_vec(m) for m in mats])


def hstack_vec(mats):
    return same_storage_fast_stack_vec([m if m[0] == CSC else to_other_storage_vec(m) for m in mats])


def bmat_vec(mats):
    mats = [list(r) for r in mats]
    assert len(mats) != 0 and len(mats[0]) != 0, "Empty stacking list"
    super_cols = len(mats[0])
    assert all(len(x) == super_cols for x in mats), "Dimension mismatch"
    assert not any(all(m is None for m in x) for x in mats), "Empty bmat row"
    assert not any(all(x[j] is None for x in mats) for j in range(super_cols)), "Empty bmat col"
    rows_per_row = [max([0] + [rows(m) for m in row if m is not None]) for row in mats]
    cols_per_col = [max([0] + [cols(row[j]) for row in mats if row[j] is not None]) for j in range(super_cols)]
    to_vstack = []
    for i, row in enumerate(mats):
        to_vstack.append(hstack_vec([zero((rows_per_row[i], cols_per_col[j])) if m is None else m for j, m in enumerate(row)]))
    return vstack_vec(to_vstack)


def kronecker_product_vec(a, b):
    if a[0] != b[0]:
        b = to_other_storage_vec(b)
    a, b = to_owned(a), to_owned(b)
    storage = a[0]
    oa, ob, inner_b = outer_dims(a), outer_dims(b), inner_dims(b)
    la, lb = np.diff(a[2]), np.diff(b[2])
    lens = np.outer(la, lb).reshape(-1)                             # slice ia * outer(b) + ib
    indptr = np.zeros(oa * ob + 1, dtype=np.int64)
    np.cumsum(lens, out=indptr[1:])
    total = int(indptr[-1])
    s = np.repeat(np.arange(oa * ob), lens)
    q = np.arange(total) - indptr[s]
    ia, ib = s // max(ob, 1), s % max(ob, 1)
    ka, kb = q // np.maximum(lb[ib], 1), q % np.maximum(lb[ib], 1)
    pa, pb = a[2][ia] + ka, b[2][ib] + kb
    with np.errstate(invalid="ignore", over="ignore"):
        values = a[4][pa] * b[4][pb]
    shape = (a[1][0] * b[1][0], a[1][1] * b[1][1])
    return (storage, shape, indptr, a[3][pa] * inner_b + b[3][pb], values)
