"""Python restatements of the reference's sparse-vector products (test infrastructure).

merge_dot / csr_mul_csvec_ref follow sprs line by line: CsVecViewI::dot_acc's merge (sprs/src/sparse/vec.rs:846-880) summed
from 0.0 with unfused products (MulAcc, mul_acc.rs:28-30), and prod::csr_mul_csvec's `val != 0` filter (prod.rs:161-184).
masked_dot_vec is the same sums, vectorised: the k-th match of every outer slice is added at once for k = 0, 1, ...  Python
floats and numpy float64 both round every product and every sum separately, so both give the reference's bits."""
import numpy as np


def merge_dot(ix, dt, vidx, vval):
    """dot_acc of one outer slice (sorted ix, dt) with a sparse vector (sorted vidx, vval): -> (sum, matched)"""
    s, matched = 0.0, False
    i = j = 0
    while i < len(ix) and j < len(vidx):
        a, b = int(ix[i]), int(vidx[j])
        if a == b:
            s = s + float(dt[i]) * float(vval[j])
            matched = True
        if a <= b:
            i += 1
        if a >= b:
            j += 1
    return s, matched


def csr_mul_csvec_ref(indptr, indices, data, rows, dim, vidx, vval, structural=False):
    """-> (result dim, indices, data).  structural=False: csr_mul_csvec (val != 0 kept; dim 0 -> empty of dim 0);
    structural=True: what mul_csr_csr gives for the same sums (every slice with a match)."""
    if dim == 0 and not structural:
        return 0, np.zeros(0, dtype=np.int64), np.zeros(0)
    oi, od = [], []
    for r in range(rows):
        s, e = int(indptr[r]), int(indptr[r + 1])
        val, matched = merge_dot(indices[s:e], data[s:e], vidx, vval)
        if (matched if structural else val != 0.0):
            oi.append(r)
            od.append(val)
    return rows, np.array(oi, dtype=np.int64), np.array(od, dtype=np.float64)


def masked_dot_vec(indptr, indices, data, rows, dim, vidx, vval, structural=False):
    """vectorised restatement of csr_mul_csvec_ref for large operands: -> (rows, indices, data, longest chain)"""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    data = np.asarray(data, dtype=np.float64)
    present = np.zeros(dim, dtype=bool)
    dense = np.zeros(dim)
    vidx = np.asarray(vidx, dtype=np.int64)
    present[vidx] = True
    dense[vidx] = np.asarray(vval, dtype=np.float64)
    hit = present[indices] if indices.size else np.zeros(0, dtype=bool)
    pos = np.nonzero(hit)[0]
    row_of = np.repeat(np.arange(rows, dtype=np.int64), np.diff(indptr))
    mrow = row_of[pos]
    prod = data[pos] * dense[indices[pos]]
    counts = np.bincount(mrow, minlength=rows) if rows else np.zeros(0, dtype=np.int64)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]]) if rows else np.zeros(0, dtype=np.int64)
    rank = np.arange(pos.size) - first[mrow] if pos.size else np.zeros(0, dtype=np.int64)
    sums = np.zeros(rows)
    order = np.argsort(rank, kind="stable")
    bounds = np.searchsorted(rank[order], np.arange(int(counts.max()) + 2 if pos.size else 1))
    for k in range(len(bounds) - 1):
        sel = order[bounds[k]:bounds[k + 1]]
        sums[mrow[sel]] = sums[mrow[sel]] + prod[sel]
    keep = counts > 0 if structural else sums != 0.0
    out = np.nonzero(keep)[0]
    return rows, out, sums[out], int(counts.max()) if pos.size else 0


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)
