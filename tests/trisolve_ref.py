"""Plain-Python restatement of the four dense-rhs triangular solves of the reference (sprs/src/sparse/linalg/trisolve.rs):
scalar float64 loops in the reference's own order — no vectorised sum that could reorder — with its singular returns, and the
number of dependency levels of a solve by the recurrence.  The GPU tests compare with these bit for bit."""
import numpy as np


class Singular(Exception):
    """Err(LinalgError::SingularMatrix(SingularMatrixInfo { index, reason })), errors.rs:59-92"""

    def __init__(self, index, reason):
        self.index, self.reason = index, reason
        super().__init__("Singular matrix at index %d (%s)" % (index, reason))


def _lists(ip, ix, dt, b):
    return [int(v) for v in ip], [int(v) for v in ix], [float(v) for v in dt], [float(v) for v in b]


def lsolve_csr_dense_rhs(n, ip, ix, dt, b):
    """trisolve.rs:30-73"""
    ip, ix, dt, x = _lists(ip, ix, dt, b)
    for r in range(n):
        diag, acc = 0.0, x[r]
        for p in range(ip[r], ip[r + 1]):
            c = ix[p]
            if c == r:
                diag = dt[p]
                continue
            if c > r:
                continue
            prod = dt[p] * x[c]
            acc = acc - prod
        if diag == 0.0:
            raise Singular(r, "diagonal element is 0")
        x[r] = acc / diag
    return np.array(x, dtype=np.float64)


def usolve_csr_dense_rhs(n, ip, ix, dt, b):
    """trisolve.rs:219-262"""
    ip, ix, dt, x = _lists(ip, ix, dt, b)
    for r in range(n - 1, -1, -1):
        diag, acc = 0.0, x[r]
        for p in range(ip[r], ip[r + 1]):
            c = ix[p]
            if c == r:
                diag = dt[p]
                continue
            if c < r:
                continue
            prod = dt[p] * x[c]
            acc = acc - prod
        if diag == 0.0:
            raise Singular(r, "diagonal element is a numeric 0")
        x[r] = acc / diag
    return np.array(x, dtype=np.float64)


def _csc_diag(ip, ix, dt, c):
    """col.get(col_ind): the stored diagonal of column c, or None"""
    for p in range(ip[c], ip[c + 1]):
        if ix[p] == c:
            return dt[p]
    return None


def lsolve_csc_dense_rhs(n, ip, ix, dt, b):
    """trisolve.rs:85-149 (ip / ix / dt: the CSC arrays)"""
    ip, ix, dt, x = _lists(ip, ix, dt, b)
    for c in range(n):
        diag = _csc_diag(ip, ix, dt, c)
        if diag is None:
            raise Singular(c, "diagonal element is a structural 0")
        if diag == 0.0:
            raise Singular(c, "diagonal element is a numeric 0")
        xc = x[c] / diag
        x[c] = xc
        for p in range(ip[c], ip[c + 1]):
            r = ix[p]
            if r <= c:
                continue
            prod = dt[p] * xc
            x[r] = x[r] - prod
    return np.array(x, dtype=np.float64)


def usolve_csc_dense_rhs(n, ip, ix, dt, b):
    """trisolve.rs:161-210 (ip / ix / dt: the CSC arrays)"""
    ip, ix, dt, x = _lists(ip, ix, dt, b)
    for c in range(n - 1, -1, -1):
        diag = _csc_diag(ip, ix, dt, c)
        if diag is None:
            raise Singular(c, "diagonal element is a structural 0")
        if diag == 0.0:
            raise Singular(c, "diagonal element is a numeric 0")
        xc = x[c] / diag
        x[c] = xc
        for p in range(ip[c], ip[c + 1]):
            r = ix[p]
            if r >= c:
                continue
            prod = dt[p] * xc
            x[r] = x[r] - prod
    return np.array(x, dtype=np.float64)


SOLVES = {"lsolve_csr": lsolve_csr_dense_rhs, "usolve_csr": usolve_csr_dense_rhs,
          "lsolve_csc": lsolve_csc_dense_rhs, "usolve_csc": usolve_csc_dense_rhs}


def levels(kind, n, ip, ix):
    """length of the longest chain of unknowns that must be solved one after the other: level(r) = 1 + max level(c) over the
    entries (r, c) of the solve's triangle (0 without any); the count is the highest level + 1"""
    if n == 0:
        return 0
    ip, ix = [int(v) for v in ip], [int(v) for v in ix]
    upper, csc = kind.startswith("u"), kind.endswith("csc")
    lv = [0] * n
    for o in (range(n - 1, -1, -1) if upper else range(n)):
        for p in range(ip[o], ip[o + 1]):
            i = ix[p]
            if csc:                       # outer o is the column: it feeds the rows on its far side
                if (i < o) if upper else (i > o):
                    lv[i] = max(lv[i], lv[o] + 1)
            elif (i > o) if upper else (i < o):
                lv[o] = max(lv[o], lv[i] + 1)
    return max(lv) + 1
