"""Restatements of the reference's recurrences for N = f32, with np.float32 scalars throughout (test infrastructure):

  lsolve_csr / usolve_csr / lsolve_csc / usolve_csc _dense_rhs   sprs/src/sparse/linalg/trisolve.rs:30-262, as tests/trisolve_ref.py
                                                                  states them for f64, entry order included (lsolve_csc scatters
                                                                  by ascending column, usolve_csc by descending column)
  gauss_seidel(mat, x, rhs, max_iter, eps)                        sprs/examples/heat.rs:103-139 instantiated for f32

Every product, every subtraction / addition and every division is ONE np.float32 operation: numpy rounds float32 (op) float32
to float32 once, as the hardware does — an f64 solve rounded at the end is not this.  `levels` is trisolve_ref's (structure only)."""
import collections

import numpy as np

import f32_ref
from trisolve_ref import Singular, levels  # noqa: F401

F = np.float32
ZERO = F(0.0)


def _lists(ip, ix, dt, b):
    assert np.asarray(dt).dtype == np.float32 and np.asarray(b).dtype == np.float32
    return [int(v) for v in ip], [int(v) for v in ix], [F(v) for v in dt], [F(v) for v in b]


def _out(x):
    return np.array(x, dtype=np.float32)


def lsolve_csr_dense_rhs(n, ip, ix, dt, b):
    """trisolve.rs:30-73"""
    ip, ix, dt, x = _lists(ip, ix, dt, b)
    with np.errstate(all="ignore"):
        for r in range(n):
            diag, acc = ZERO, x[r]
            for p in range(ip[r], ip[r + 1]):
                c = ix[p]
                if c == r:
                    diag = dt[p]
                    continue
                if c > r:
                    continue
                prod = F(dt[p] * x[c])
                acc = F(acc - prod)
            if diag == ZERO:
                raise Singular(r, "diagonal element is 0")
            x[r] = F(acc / diag)
    return _out(x)


def usolve_csr_dense_rhs(n, ip, ix, dt, b):
    """trisolve.rs:219-262"""
    ip, ix, dt, x = _lists(ip, ix, dt, b)
    with np.errstate(all="ignore"):
        for r in range(n - 1, -1, -1):
            diag, acc = ZERO, x[r]
            for p in range(ip[r], ip[r + 1]):
                c = ix[p]
                if c == r:
                    diag = dt[p]
                    continue
                if c < r:
                    continue
                prod = F(dt[p] * x[c])
                acc = F(acc - prod)
            if diag == ZERO:
                raise Singular(r, "diagonal element is a numeric 0")
            x[r] = F(acc / diag)
    return _out(x)


def _csc_diag(ip, ix, dt, c):
    """col.get(col_ind): the stored diagonal of column c, or None"""
    for p in range(ip[c], ip[c + 1]):
        if ix[p] == c:
            return dt[p]
    return None


def _solve_csc(n, ip, ix, dt, b, upper):
    ip, ix, dt, x = _lists(ip, ix, dt, b)
    with np.errstate(all="ignore"):
        for c in (range(n - 1, -1, -1) if upper else range(n)):
            diag = _csc_diag(ip, ix, dt, c)
            if diag is None:
                raise Singular(c, "diagonal element is a structural 0")
            if diag == ZERO:
                raise Singular(c, "diagonal element is a numeric 0")
            xc = F(x[c] / diag)
            x[c] = xc
            for p in range(ip[c], ip[c + 1]):
                r = ix[p]
                if (r >= c) if upper else (r <= c):
                    continue
                prod = F(dt[p] * xc)
                x[r] = F(x[r] - prod)
    return _out(x)


def lsolve_csc_dense_rhs(n, ip, ix, dt, b):
    """trisolve.rs:85-149 (ip / ix / dt: the CSC arrays): columns 0 .. n-1, every row receives its products by ascending column"""
    return _solve_csc(n, ip, ix, dt, b, False)


def usolve_csc_dense_rhs(n, ip, ix, dt, b):
    """trisolve.rs:161-210 (ip / ix / dt: the CSC arrays): columns n-1 .. 0, every row receives its products by descending column"""
    return _solve_csc(n, ip, ix, dt, b, True)


SOLVES = {"lsolve_csr": lsolve_csr_dense_rhs, "usolve_csr": usolve_csr_dense_rhs,
          "lsolve_csc": lsolve_csc_dense_rhs, "usolve_csc": usolve_csc_dense_rhs}


class NoDiagonal(Exception):
    """`diag.unwrap()` of None, heat.rs:126"""


def ndarray_sum(xs):
    """`.sum()` of a contiguous ndarray (numeric_util::unrolled_fold): eight interleaved partial sums over blocks of eight, combined
    as ((((0 + (p0+p4)) + (p1+p5)) + (p2+p6)) + (p3+p7)), then the trailing elements one by one — in f32"""
    xs = [F(v) for v in xs]
    p = [ZERO] * 8
    full = len(xs) // 8 * 8
    for i in range(0, full, 8):
        for k in range(8):
            p[k] = F(p[k] + xs[i + k])
    acc = ZERO
    for k in range(4):
        acc = F(acc + F(p[k] + p[k + 4]))
    for v in xs[full:]:
        acc = F(acc + v)
    return acc


def residual_sum(shape, ip, ix, dt, x, rhs):
    """(&mat * &x - rhs).sum(), heat.rs:112, 131: the f32 SpMV chain of f32_ref, one subtraction per row, ndarray's sum"""
    v = f32_ref.mul_vec(shape, np.asarray(ip), np.asarray(ix), dt, x)
    return ndarray_sum(v - rhs)


GsResult = collections.namedtuple("GsResult", "x iterations converged error sums errors")


def gauss_seidel(shape, ip, ix, dt, x0, rhs, max_iter, eps, on_sweep=None):
    """heat.rs:103-139 for f32 -> GsResult(x, iterations, converged, error, ...): Ok((it, error)) is converged with
    iterations = it, Err(error) is not converged with iterations = max_iter.  `sums` / `errors` list the residual sum and its
    square root for the start vector and after every sweep; on_sweep(k, x) sees the iterate they were computed from."""
    assert dt.dtype == np.float32 and x0.dtype == np.float32 and rhs.dtype == np.float32
    n = shape[0]
    eps = F(eps)
    lip, lix, ldt = [int(v) for v in ip], [int(v) for v in ix], [F(v) for v in dt]
    x = [F(v) for v in x0]
    b = [F(v) for v in rhs]
    sums, errors = [], []

    def error_of(k):
        xa = _out(x)
        if on_sweep:
            on_sweep(k, xa)
        sums.append(residual_sum(shape, ip, ix, dt, xa, rhs))
        errors.append(F(np.sqrt(sums[-1])))
        return errors[-1]

    with np.errstate(all="ignore"):
        error = error_of(0)
        for it in range(max_iter):
            for r in range(n):
                sigma, diag = ZERO, None
                for p in range(lip[r], lip[r + 1]):
                    c = lix[p]
                    if c != r:
                        prod = F(ldt[p] * x[c])
                        sigma = F(sigma + prod)
                    else:
                        diag = ldt[p]
                if diag is None:
                    raise NoDiagonal(r)
                x[r] = F(F(b[r] - sigma) / diag)
            error = error_of(it + 1)
            if error < eps:
                return GsResult(_out(x), it, True, error, sums, errors)
    return GsResult(_out(x), max_iter, False, error, sums, errors)
