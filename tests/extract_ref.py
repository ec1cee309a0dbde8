"""Python restatements of the reference's matrix extraction (test infrastructure): CsMat::outer_view (sprs/src/sparse/csmat.rs:
1219-1231), diag (1234-1256), nnz_index (1312-1351) and to_inner_onehot (1017-1056) on the raw (indptr, indices, data) of a
compressed matrix; `outer` slices, whatever the storage."""
import numpy as np


def outer_view(indptr, indices, data, i):
    """-> (indices, data) of slice i, or None past the last one"""
    if i >= len(indptr) - 1:
        return None
    s, e = int(indptr[i]), int(indptr[i + 1])
    return np.asarray(indices[s:e]), np.asarray(data[s:e])


def nnz_index_outer_inner(indptr, indices, outer, inner):
    """-> the global position of (outer, inner) or None"""
    if outer >= len(indptr) - 1:
        return None
    s, e = int(indptr[outer]), int(indptr[outer + 1])
    sl = np.asarray(indices[s:e], dtype=np.uint64)
    j = int(np.searchsorted(sl, np.uint64(inner)))
    return s + j if j < len(sl) and int(sl[j]) == int(inner) else None


def nnz_index(indptr, indices, csc, row, col):
    return nnz_index_outer_inner(indptr, indices, col, row) if csc else nnz_index_outer_inner(indptr, indices, row, col)


def diag(shape, indptr, indices, data):
    """-> (dim, indices, data): entry i is stored iff (i, i) is (the same walk for CSR and CSC)"""
    n = min(shape)
    oi, od = [], []
    for i in range(n):
        p = nnz_index_outer_inner(indptr, indices, i, i)
        if p is not None:
            oi.append(i)
            od.append(data[p])
    return n, np.array(oi, dtype=np.int64), np.array(od, dtype=np.float64)


def to_inner_onehot(indptr, indices, data):
    """-> (indptr, indices, data).  Iterator::max_by over the non-NaN entries returns the LAST of equal maxima; partial_cmp
    holds -0.0 and +0.0 equal."""
    oip, oix = [0], []
    for o in range(len(indptr) - 1):
        best = None
        for e in range(int(indptr[o]), int(indptr[o + 1])):
            x = float(data[e])
            if x != x:
                continue
            if best is None or x >= best[0]:
                best = (x, int(indices[e]))
        if best is not None:
            oix.append(best[1])
        oip.append(len(oix))
    return np.array(oip, dtype=np.int64), np.array(oix, dtype=np.int64), np.ones(len(oix))
