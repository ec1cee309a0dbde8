"""CPU restatement of the dense <-> sparse boundary of sprs for the tests: csr_from_dense / csc_from_dense (csmat.rs:499-549),
assign_to_dense / to_dense (to_dense.rs:12-30, csmat.rs:1127-1134), csmat_binop_dense_raw with the closures of
add_dense_mat_same_ordering / mul_dense_mat_same_ordering (binop.rs:273-433) and `&CsMat + &Array2` (csmat.rs:1951-1987) — line
by line, and numpy twins for larger inputs (numpy does not fuse a multiply and an add).  A sparse matrix is (storage, shape,
indptr, indices, data) with storage 0 = CSR, 1 = CSC as in construct_ref.py; a dense matrix is a 2-D numpy array and, where the
reference looks at its fastest axis, an order "C" (Axis(1) fastest) or "F" (Axis(0)).  Where the reference asserts or panics,
these raise AssertionError with its text."""
import numpy as np

from construct_ref import (CSC, CSR, bits, inner_dims, mat, nnz, outer_dims, outer_iterator, same_mat, to_other_storage,  # noqa: F401
                           to_other_storage_vec, to_owned, transpose)

ADD, MUL = "add", "mul"


def same_dense(got, want):
    """equal shapes and equal value BITS"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and np.array_equal(bits(got), bits(want))


def clamp(epsilon):
    """csmat.rs:506-510: `if epsilon > N::zero() { epsilon } else { N::zero() }` — a NaN or negative epsilon is 0"""
    epsilon = float(epsilon)
    return epsilon if epsilon > 0.0 else 0.0


# ---- csmat.rs:499-549 ----------------------------------------------------------------------------------------------------------

def csr_from_dense(m, epsilon):
    m = np.asarray(m, dtype=np.float64)
    epsilon = clamp(epsilon)
    nrows, ncols = m.shape
    indptr = [0] * (nrows + 1)
    count = 0
    for r in range(nrows):
        count += sum(1 for x in m[r] if abs(float(x)) > epsilon)
        indptr[r + 1] = count
    indices, data = [], []
    for r in range(nrows):
        for col_ind, x in enumerate(m[r]):
            if abs(float(x)) > epsilon:
                indices.append(col_ind)
                data.append(x)
    return mat(CSR, (nrows, ncols), indptr, indices, data)


def csc_from_dense(m, epsilon):
    """Self::csr_from_dense(m.reversed_axes(), epsilon).transpose_into()"""
    return transpose(csr_from_dense(np.asarray(m, dtype=np.float64).T, epsilon))


def from_dense(m, epsilon, storage):
    return csr_from_dense(m, epsilon) if storage == CSR else csc_from_dense(m, epsilon)


def from_dense_vec(m, epsilon, storage):
    m = np.asarray(m, dtype=np.float64)
    lines = m if storage == CSR else m.T
    keep = np.abs(lines) > clamp(epsilon)
    indptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    idx = np.nonzero(keep)                                           # line by line, ascending inside a line
    return (storage, m.shape, indptr, idx[1].astype(np.int64), lines[idx])


# ---- to_dense.rs:12-30, csmat.rs:1127-1134 -------------------------------------------------------------------------------------

def assign_to_dense(array, spmat):
    """in place; the array is not zeroed first"""
    assert spmat[1][1] == array.shape[1], "Dimension mismatch"
    assert spmat[1][0] == array.shape[0], "Dimension mismatch"
    view = array.view(np.uint64)                                     # N: Clone — the bits move
    for o, sprow in enumerate(outer_iterator(spmat)):
        for ind, val in sprow:
            at = (o, ind) if spmat[0] == CSR else (ind, o)
            view[at] = np.float64(val).view(np.uint64)
    return array


def to_dense(spmat):
    return assign_to_dense(np.zeros(spmat[1]), spmat)


def assign_to_dense_vec(array, spmat):
    assert spmat[1][1] == array.shape[1], "Dimension mismatch"
    assert spmat[1][0] == array.shape[0], "Dimension mismatch"
    m = to_owned(spmat)
    outer_of = np.repeat(np.arange(outer_dims(m)), np.diff(m[2]))
    at = (outer_of, m[3]) if m[0] == CSR else (m[3], outer_of)
    array.view(np.uint64)[at] = bits(m[4])
    return array


def to_dense_vec(spmat):
    return assign_to_dense_vec(np.zeros(spmat[1]), spmat)


# ---- binop.rs:273-433 ----------------------------------------------------------------------------------------------------------

def closure(op, alpha, beta=1.0):
    """|x, y| &alpha * x + &beta * y (binop.rs:319) / |x, y| alpha * x * y (binop.rs:367): unfused float64 arithmetic"""
    alpha, beta = np.float64(alpha), np.float64(beta)
    if op == ADD:
        return lambda x, y: alpha * np.float64(x) + beta * np.float64(y)
    assert op == MUL
    return lambda x, y: alpha * np.float64(x) * np.float64(y)


def csmat_binop_dense_raw(lhs, rhs, binop, out, rhs_order="C", out_order="C"):
    """binop.rs:384-433; out is written in place"""
    if lhs[1][1] != rhs.shape[1] or lhs[1][1] != out.shape[1] or lhs[1][0] != rhs.shape[0] or lhs[1][0] != out.shape[0]:
        raise AssertionError("Dimension mismatch")
    if (lhs[0], rhs_order, out_order) not in ((CSR, "C", "C"), (CSC, "F", "F")):
        raise AssertionError("Storage mismatch")
    zero = np.float64(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for o, lrow in enumerate(outer_iterator(lhs)):
            rrow = rhs[o, :] if lhs[0] == CSR else rhs[:, o]
            orow = out[o, :] if lhs[0] == CSR else out[:, o]
            stored = dict(lrow)
            # nnz_or_zip of the enumerated dense line (every index) with the sparse line: Left = dense only, Both; Right never
            # happens for a validated matrix
            for i in range(rrow.shape[0]):
                orow[i] = binop(stored[i], rrow[i]) if i in stored else binop(zero, rrow[i])
    return out


def add_dense_mat_same_ordering(lhs, rhs, alpha, beta, order="C"):
    """binop.rs:279-323: the result has rhs' fastest axis"""
    res = np.zeros(rhs.shape, order=order)
    return csmat_binop_dense_raw(lhs, rhs, closure(ADD, alpha, beta), res, order, order)


def mul_dense_mat_same_ordering(lhs, rhs, alpha, order="C"):
    """binop.rs:331-371"""
    res = np.zeros(rhs.shape, order=order)
    return csmat_binop_dense_raw(lhs, rhs, closure(MUL, alpha), res, order, order)


def add_dense(lhs, rhs, order="C"):
    """`&lhs + &rhs` (csmat.rs:1951-1987)"""
    if (lhs[0] == CSR) == (order == "C"):
        return add_dense_mat_same_ordering(lhs, rhs, 1.0, 1.0, order)
    return add_dense_mat_same_ordering(to_other_storage(to_owned(lhs)), rhs, 1.0, 1.0, order)


def binop_dense_vec(lhs, rhs, op, alpha, beta=1.0):
    """the numpy twin of csmat_binop_dense_raw with closure(op, alpha, beta): l is +0.0 where lhs stores nothing"""
    if lhs[1] != tuple(rhs.shape):
        raise AssertionError("Dimension mismatch")
    l = to_dense_vec(lhs)
    alpha, beta = np.float64(alpha), np.float64(beta)
    with np.errstate(invalid="ignore", over="ignore"):
        al = alpha * l
        return al + beta * rhs if op == ADD else al * rhs
