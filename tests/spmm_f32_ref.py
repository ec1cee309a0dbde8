"""Numpy restatement of the reference's dense products for N = f32 (test infrastructure):

  csr_mulacc_dense_rowmaj   prod.rs:189-214 — per out[i, j] the left-to-right chain acc = f32(acc + f32(a * b)) over the entries
                            of row i in order, starting from out[i, j] (MulAcc for a float, mul_acc.rs:17-31: `*self += a * b`)
  result_col_major          csmat.rs:2002-2045 — `&CsMat * &Array2` allocates Array::zeros((rows, cols)) for >= 8 columns and
                            Array::zeros((rows, cols).f()) below, in both storages

The chain is evaluated for all rows at once, entry position by entry position: rows sorted by length, so that the rows that
still have a t-th entry are a prefix.  Every intermediate is a float32 array: numpy rounds float32 (op) float32 to float32
once, as the hardware does."""
import numpy as np

import f32_ref

F = np.float32


def csr_mulacc_dense_rowmaj(shape, indptr, indices, data, rhs, out, max_len=None):
    """out[i, :] += sum_k a_ik rhs[k, :] in place, left to right; returns out.  Rows of more than max_len entries (None: no
    limit) are left alone.  data, rhs, out: float32."""
    assert data.dtype == np.float32 and rhs.dtype == np.float32 and out.dtype == np.float32
    assert rhs.shape[0] == shape[1] and out.shape == (shape[0], rhs.shape[1])
    ip = np.asarray(indptr).astype(np.int64)
    ix = np.asarray(indices).astype(np.int64)
    lens = np.diff(ip)
    order = np.argsort(-lens, kind="stable")
    if max_len is not None:
        order = order[lens[order] <= max_len]
    order = order[lens[order] > 0]                   # an empty row keeps its bits (prod.rs:203: the loop body never runs)
    if order.size == 0 or rhs.shape[1] == 0:
        return out
    sl = lens[order]                                 # descending
    acc = out[order].copy()
    start = ip[order]
    for t in range(int(sl[0])):
        n = int(np.searchsorted(-sl, -t, side="left"))           # rows with more than t entries
        pos = start[:n] + t
        p = data[pos][:, None] * rhs[ix[pos]]                      # each product rounded to f32
        acc[:n] = acc[:n] + p
    out[order] = acc
    return out


def mul_dense(shape, indptr, indices, data, rhs, max_len=None):
    """`&A * &B`: the accumulate form on a zeroed result (csmat.rs:2004)"""
    return csr_mulacc_dense_rowmaj(shape, indptr, indices, data, rhs, np.zeros((shape[0], rhs.shape[1]), dtype=np.float32), max_len)


def result_col_major(k):
    """the layout `&CsMat * &Array2` allocates for a rhs of k columns (csmat.rs:2002-2045)"""
    return k < 8


def mul_vec_columns(shape, indptr, indices, data, rhs):
    """column by column through the SpMV chain of f32_ref (csr_mulacc_dense_colmaj, prod.rs:274-298)"""
    return np.stack([f32_ref.mul_vec(shape, indptr, indices, data, np.ascontiguousarray(rhs[:, j])) for j in range(rhs.shape[1])], axis=1)
