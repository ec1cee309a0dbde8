"""Numpy restatements of the reference for N = f32, with np.float32 scalars throughout (test infrastructure):

  mul_acc_mat_vec_csr   prod.rs:103-127 — per row the left-to-right chain acc = acc + (a * x), the product rounded to f32
                        before the add (MulAcc for a float, mul_acc.rs:17-31: `*self += a * b`)
  BiCGSTAB              bicgstab.rs:117-229 (new / step / soft_restart / hard_restart / solve), dense vectors (the reference's
                        CsVec arithmetic on vectors without structural zeros), serial dots from 0 (vec.rs:846-880, 907-918)

Every intermediate is an np.float32: numpy rounds float32 (op) float32 to float32 once, as the hardware does."""
import numpy as np

F = np.float32


def mul_acc_mat_vec_csr(shape, indptr, indices, data, x, y):
    """y[r] += sum_k a_rk x_k in place, left to right; returns y.  data, x, y: float32 arrays."""
    assert data.dtype == np.float32 and x.dtype == np.float32 and y.dtype == np.float32
    rows = shape[0]
    for r in range(rows):
        lo, hi = int(indptr[r]), int(indptr[r + 1])
        if hi == lo:
            continue
        acc = y[r]
        prods = data[lo:hi] * x[indices[lo:hi].astype(np.int64)]      # each rounded to f32
        for p in prods:
            acc = F(acc + p)
        y[r] = acc
    return y


def mul_vec(shape, indptr, indices, data, x):
    """`&A * &x`: the accumulate form on a zeroed result (csmat.rs:2119-2160)"""
    return mul_acc_mat_vec_csr(shape, indptr, indices, data, x, np.zeros(shape[0], dtype=np.float32))


def dot(a, b):
    s = F(0.0)
    for p in a * b:
        s = F(s + p)
    return s


def l2_norm(a):
    return F(np.sqrt(dot(a, a)))


class BiCGSTAB:
    """bicgstab.rs:117-229 for f32; `a` is a CSR triple (shape, indptr, indices, data)."""

    def __init__(self, a, x0, b, soft_restart_threshold=0.1):
        self.a, self.b = a, b.astype(np.float32)
        self.x = x0.astype(np.float32).copy()
        self.r = self.b - mul_vec(*a, self.x)
        self.rhat = self.r.copy()
        self.p = self.r.copy()
        self.err = l2_norm(self.r)
        self.rho = F(self.err * self.err)
        self.iteration_count = self.soft_restart_count = self.hard_restart_count = 0
        self.soft_restart_threshold = F(soft_restart_threshold)

    def soft_restart(self):
        self.soft_restart_count += 1
        self.rhat = self.r.copy()
        self.rho = F(self.err * self.err)
        self.p = self.r.copy()

    def hard_restart(self):
        self.hard_restart_count += 1
        self.r = self.b - mul_vec(*self.a, self.x)
        self.err = l2_norm(self.r)
        self.soft_restart()
        self.soft_restart_count -= 1

    def step(self):
        self.iteration_count += 1
        with np.errstate(all="ignore"):
            v = mul_vec(*self.a, self.p)
            alpha = F(self.rho / dot(self.rhat, v))
            h = self.x + self.p * alpha
            s = self.r - v * alpha
            t = mul_vec(*self.a, s)
            omega = F(dot(t, s) / dot(t, t))
            self.x = h + omega * s
            self.r = s - t * omega
            self.err = l2_norm(self.r)
            rho_prev = self.rho
            self.rho = dot(self.rhat, self.r)
            if F(np.abs(self.rho) / F(self.err * self.err)) < self.soft_restart_threshold:
                self.soft_restart()
            else:
                beta = F(F(self.rho / rho_prev) * F(alpha / omega))
                self.p = self.r + (self.p - v * omega) * beta
        return self.err

    @classmethod
    def solve(cls, a, x0, b, tol, max_iter, soft_restart_threshold=0.1):
        """-> (solver, converged): Ok(solver) / Err(solver) of the reference"""
        tol = F(tol)
        solver = cls(a, x0, b, soft_restart_threshold)
        for _ in range(max_iter):
            solver.step()
            if solver.err < tol:
                solver.hard_restart()
                if solver.err < tol:
                    return solver, True
        return solver, False


def csc_to_csr(shape, indptr, indices, data):
    """to_other_storage on the host (counting sort: rows ascending inside every output row)"""
    rows, cols = shape
    order = np.argsort(indices.astype(np.int64), kind="stable")
    col_of = np.repeat(np.arange(cols, dtype=np.int64), np.diff(indptr.astype(np.int64)))
    out_ptr = np.zeros(rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(indices.astype(np.int64), minlength=rows), out=out_ptr[1:])
    return shape, out_ptr, col_of[order], data[order]


# the reference's own test system (test_bicgstab_f32, bicgstab.rs:313-350): 4 x 4 CSC, b = x0 = 1, tol = 1e-18, max_iter = 50
REF_SYSTEM_CSC = ((4, 4), np.array([0, 2, 4, 6, 8], dtype=np.uint64), np.array([0, 3, 1, 2, 1, 2, 0, 3], dtype=np.uint64),
                  np.array([1.0, 2.0, 21.0, 6.0, 6.0, 2.0, 2.0, 8.0], dtype=np.float32))
REF_TOL, REF_MAX_ITER = 1e-18, 50
