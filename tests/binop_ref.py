"""Python restatements of the reference's sparse binops (test infrastructure).

csmat_binop_ref / csvec_binop_ref follow sprs line by line: the nnz_or_zip merge of two sorted index lists with the operation
applied to (l, +0.0), (+0.0, r) or (l, r), csmat_binop_same_storage_raw's `!val.is_zero()` filter (binop.rs:229-271) and
csvec_binop's unconditional append after csvec_fix_zeros (binop.rs:442-479).  csmat_binop_vec / csvec_binop_vec are the same
operations vectorised with numpy: the union of the (outer, inner) keys, both operands scattered over +0.0, one elementwise
operation.  Python floats and numpy float64 both perform exactly one IEEE operation per entry, so all give the reference's bits."""
import numpy as np

ADD, SUB, MUL = 0, 1, 2


def apply(op, l, r):
    if op == ADD:
        return l + r
    if op == SUB:
        return l - r
    return l * r


def nnz_or_zip(li, lv, ri, rv):
    """the merge of two sorted (index, value) lists: yields (index, l or None, r or None), an equal index once"""
    i = j = 0
    while i < len(li) or j < len(ri):
        if j >= len(ri) or (i < len(li) and int(li[i]) < int(ri[j])):
            yield int(li[i]), float(lv[i]), None
            i += 1
        elif i >= len(li) or int(ri[j]) < int(li[i]):
            yield int(ri[j]), None, float(rv[j])
            j += 1
        else:
            yield int(li[i]), float(lv[i]), float(rv[j])
            i += 1
            j += 1


def csmat_binop_ref(a, b, op):
    """a, b = (shape, indptr, indices, data) in the same storage -> (shape, indptr, indices, data) of csmat_binop"""
    (shape, aip, aix, adt), (bshape, bip, bix, bdt) = a, b
    assert tuple(shape) == tuple(bshape), "Dimension mismatch"
    outer = len(aip) - 1
    assert len(bip) - 1 == outer, "Storage mismatch"
    oip, oix, odt = [0], [], []
    for r in range(outer):
        s0, e0, s1, e1 = int(aip[r]), int(aip[r + 1]), int(bip[r]), int(bip[r + 1])
        for ind, l, rr in nnz_or_zip(aix[s0:e0], adt[s0:e0], bix[s1:e1], bdt[s1:e1]):
            val = apply(op, 0.0 if l is None else l, 0.0 if rr is None else rr)
            if not (val == 0.0):
                oix.append(ind)
                odt.append(val)
        oip.append(len(oix))
    return tuple(shape), np.array(oip, dtype=np.int64), np.array(oix, dtype=np.int64), np.array(odt, dtype=np.float64)


def csvec_binop_ref(v, w, op):
    """v, w = (dim, indices, data) -> (dim, indices, data) of csvec_binop; AssertionError("Dimension mismatch") as the reference"""
    (vd, vi, vv), (wd, wi, wv) = v, w
    if wd == 0:
        wd = vd
    if vd == 0:
        vd = wd
    assert vd == wd, "Dimension mismatch"
    oi, od = [], []
    for ind, l, r in nnz_or_zip(vi, vv, wi, wv):
        oi.append(ind)
        od.append(apply(op, 0.0 if l is None else l, 0.0 if r is None else r))
    return vd, np.array(oi, dtype=np.int64), np.array(od, dtype=np.float64)


def _merge_vec(ka, va, kb, vb, op):
    keys = np.union1d(ka, kb)
    l = np.zeros(keys.size)
    r = np.zeros(keys.size)
    l[np.searchsorted(keys, ka)] = va
    r[np.searchsorted(keys, kb)] = vb
    with np.errstate(invalid="ignore"):           # inf - inf, inf * 0.0: NaN is the expected value
        return keys, apply(op, l, r)


def csmat_binop_vec(a, b, op):
    """vectorised twin of csmat_binop_ref for large operands"""
    (shape, aip, aix, adt), (bshape, bip, bix, bdt) = a, b
    assert tuple(shape) == tuple(bshape), "Dimension mismatch"
    outer = len(aip) - 1
    inner = max(int(shape[0]), int(shape[1]), 1)
    aip, bip = np.asarray(aip, dtype=np.int64), np.asarray(bip, dtype=np.int64)
    ka = np.repeat(np.arange(outer, dtype=np.int64), np.diff(aip)) * inner + np.asarray(aix, dtype=np.int64)
    kb = np.repeat(np.arange(outer, dtype=np.int64), np.diff(bip)) * inner + np.asarray(bix, dtype=np.int64)
    keys, val = _merge_vec(ka, np.asarray(adt, dtype=np.float64), kb, np.asarray(bdt, dtype=np.float64), op)
    keep = ~(val == 0.0)
    keys, val = keys[keep], val[keep]
    oip = np.zeros(outer + 1, dtype=np.int64)
    if outer:
        np.cumsum(np.bincount(keys // inner, minlength=outer), out=oip[1:])
    return tuple(shape), oip, keys % inner, val


def csvec_binop_vec(v, w, op):
    (vd, vi, vv), (wd, wi, wv) = v, w
    if wd == 0:
        wd = vd
    if vd == 0:
        vd = wd
    assert vd == wd, "Dimension mismatch"
    keys, val = _merge_vec(np.asarray(vi, dtype=np.int64), np.asarray(vv, dtype=np.float64), np.asarray(wi, dtype=np.int64),
                           np.asarray(wv, dtype=np.float64), op)
    return vd, keys, val


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def same_mat(got, want):
    """shape, indptr, indices equal; values equal BIT FOR BIT"""
    return (tuple(got[0]) == tuple(want[0]) and np.array_equal(np.asarray(got[1], dtype=np.int64), np.asarray(want[1], dtype=np.int64))
            and np.array_equal(np.asarray(got[2], dtype=np.int64), np.asarray(want[2], dtype=np.int64))
            and np.array_equal(bits(got[3]), bits(want[3])))


def same_vec(got, want):
    return (int(got[0]) == int(want[0]) and np.array_equal(np.asarray(got[1], dtype=np.int64), np.asarray(want[1], dtype=np.int64))
            and np.array_equal(bits(got[2]), bits(want[2])))
