"""numpy restatement of the reference's structure checks and unsorted constructors — no device:
  utils::check_compressed_structure   sprs/src/sparse.rs:300-358 (with IndPtrBase::check_structure, indptr.rs:37-74)
  CsMat::new_from_unsorted(_csc)      csmat.rs:311-401
  CsVec::try_new / new_from_unsorted  vec.rs:440-491, 536-557
Index arrays are taken as unsigned at their own width, as the device entry points read them (a negative value of a signed array
is a large index)."""
import numpy as np

CSR, CSC = 0, 1
OK, UNSORTED, SIZE_MISMATCH, OUT_OF_RANGE = 0, 1, 2, 3     # StructureErrorKind (errors.rs)
NO_OUTER = (1 << 64) - 1
GOOD = (OK, "", 0)


def _unsigned(a):
    a = np.asarray(a)
    if a.dtype.kind == "i":
        return a.view(np.dtype("u%d" % a.dtype.itemsize))
    return a


def _sorted(ix):
    return bool(np.all(ix[1:] > ix[:-1]))


def check_indptr(outer, indptr, nnz, iptr_bits=64):
    """the findings about the indptr alone, in the reference's order; None when it is sound"""
    ip = [int(v) for v in _unsigned(indptr)]
    if len(ip) != outer + 1:
        return (SIZE_MISMATCH, "Indptr length does not match dimension", NO_OUTER)
    if outer + 1 > (1 << iptr_bits) - 1:
        return (OUT_OF_RANGE, "Iptr type not large enough for this matrix", NO_OUTER)
    if any(b < a for a, b in zip(ip, ip[1:])):
        return (UNSORTED, "Unsorted indptr", NO_OUTER)
    if ip[-1] > (1 << 63) - 1:
        return (OUT_OF_RANGE, "An indptr value is larger than allowed", NO_OUTER)
    if ip[-1] - ip[0] != nnz:
        return (SIZE_MISMATCH, "Indices length and inpdtr's nnz do not match", NO_OUTER)
    return None


def check_compressed_structure(inner, outer, indptr, indices, idx_bits=64, iptr_bits=64):
    """-> (kind, text, outer): the first finding in the reference's order, GOOD when there is none.  `outer` is the first
    offending outer slice, NO_OUTER for a finding about the dimensions or the indptr."""
    ix = _unsigned(indices)
    if len(np.asarray(indptr)) != outer + 1:
        return (SIZE_MISMATCH, "Indptr length does not match dimension", NO_OUTER)
    if inner > (1 << idx_bits) - 1:
        return (OUT_OF_RANGE, "Index type not large enough for this matrix", NO_OUTER)
    bad = check_indptr(outer, indptr, len(ix), iptr_bits)
    if bad:
        return bad
    ip = [int(v) for v in _unsigned(indptr)]
    for r in range(outer):
        row = ix[ip[r] - ip[0]:ip[r + 1] - ip[0]]
        if not _sorted(row):
            return (UNSORTED, "Indices are not sorted", r)
        if row.size and int(row[-1]) >= inner:
            return (OUT_OF_RANGE, "Indice is larger than inner dimension", r)
    return GOOD


def new_from_unsorted(storage, shape, indptr, indices, data):
    """-> ((kind, text, outer), (shape, indptr, indices, data) or None): every outer slice that is not sorted is sorted by index
    (its values travel with their indices, bit for bit), sorted slices are skipped, then the whole is checked"""
    inner, outer = (shape[1], shape[0]) if storage == CSR else (shape[0], shape[1])
    ix = np.array(_unsigned(indices), copy=True)
    dt = np.array(np.asarray(data, dtype=np.float64), copy=True)
    if ix.size != dt.size:
        return (SIZE_MISMATCH, "data and indices have different sizes", NO_OUTER), None
    bad = check_indptr(outer, indptr, ix.size)     # (the reference would index out of bounds and panic: csmat.rs:337-340)
    if bad:
        return bad, None
    ip = [int(v) for v in _unsigned(indptr)]
    bits = dt.view(np.uint64)
    for r in range(outer):
        s, e = ip[r] - ip[0], ip[r + 1] - ip[0]
        if _sorted(ix[s:e]):
            continue
        order = np.argsort(ix[s:e], kind="stable")
        ix[s:e] = ix[s:e][order]
        bits[s:e] = bits[s:e][order]
    res = check_compressed_structure(inner, outer, indptr, ix)
    if res[0] != OK:
        return res, None
    return GOOD, (tuple(shape), np.array(indptr, copy=True), ix, dt)


def check_vec(dim, indices, idx_bits=64):
    """CsVec::try_new's findings -> (kind, text, 0)"""
    ix = _unsigned(indices)
    if dim > (1 << idx_bits) - 1:
        return (OUT_OF_RANGE, "Index size is too small", 0)
    if not _sorted(ix):
        return (UNSORTED, "Unsorted indices", 0)
    if ix.size and int(ix[-1]) >= dim:
        return (SIZE_MISMATCH, "indices larger than vector size", 0)
    return GOOD


def vec_new_from_unsorted(dim, indices, data):
    """-> ((kind, text, 0), (dim, indices, data) or None): check, sort only on Unsorted, check again"""
    ix = np.array(_unsigned(indices), copy=True)
    dt = np.array(np.asarray(data, dtype=np.float64), copy=True)
    res = check_vec(dim, ix)
    if res[0] == UNSORTED:
        order = np.argsort(ix, kind="stable")
        ix = ix[order]
        dt = dt.view(np.uint64)[order].view(np.float64)
        res = check_vec(dim, ix)
    if res[0] != OK:
        return res, None
    return GOOD, (dim, ix, dt)


def same_mat(got, want):
    """indptr, indices and the uint64 view of the values, bit for bit"""
    return (tuple(got[0]) == tuple(want[0]) and np.array_equal(np.asarray(got[1]).astype(np.uint64), np.asarray(want[1]).astype(np.uint64))
            and np.array_equal(np.asarray(got[2]).astype(np.uint64), np.asarray(want[2]).astype(np.uint64))
            and np.array_equal(np.asarray(got[3], dtype=np.float64).view(np.uint64), np.asarray(want[3], dtype=np.float64).view(np.uint64)))
