"""Restatement of sprs-ldl (sprs-ldl/src/lib.rs) in plain Python, written from the reference's text for the tests: the oracle of
tests/test_ldl_cpu.py, tests/test_ldl_gpu.py and the emulator run.

Two formulations of the numeric pass:
  numeric_sequential   the loop of ldl_numeric (lib.rs:502-593) statement by statement, with the double stack of
                       sprs/src/stack.rs (push_left, push_left_on_right, iter_right) written out
  numeric_closed       what the kernels implement: the structure of L from the parents alone, every row's pattern ordered by the
                       closed form (t descending, i ascending) with t(i) = the first stored entry whose climb reaches i, values
                       scattered into the column form that the symbolic pass laid out
and numeric_closed(..., ascending=True), which walks every pattern by ascending index instead: used only to show that a case is
sensitive to the order.

A matrix is (n, indptr, indices, data) in the handle's own storage: everything walks the outer dimension (outer_iterator_papt,
csmat.rs:1170-1185) and maps inner indices through perm_inv (iter_perm(perm.inv()), vec.rs:651-662).  Python floats are IEEE
doubles and `a - b * c` rounds the product, then the difference, as the reference's `*yw - *lx * yi` does."""
import numpy as np


class Singular(Exception):
    """LinalgError::SingularMatrix (lib.rs:585-590)"""

    def __init__(self, index):
        super().__init__("Singular matrix at index %d (diagonal element is a numeric 0)" % index)
        self.index = index


def inverse(perm):
    inv = [0] * len(perm)
    for i, p in enumerate(perm):
        inv[p] = i
    return inv


def _perms(n, perm):
    if perm is None:
        return list(range(n)), list(range(n))
    perm = [int(p) for p in perm]
    return perm, inverse(perm)


def symbolic(n, indptr, indices, perm=None):
    """ldl_symbolic (lib.rs:445-496) without the symmetry check: (parents with None for a root, l_nz, l_colptr)"""
    perm, pinv = _perms(n, perm)
    parents = [None] * n
    l_nz = [0] * n
    flag = [0] * n
    for k in range(n):
        flag[k] = k
        parents[k] = None                                   # set_root
        l_nz[k] = 0
        o = perm[k]
        for p in range(int(indptr[o]), int(indptr[o + 1])):
            i = pinv[int(indices[p])]
            if i < k:
                while flag[i] != k:
                    if parents[i] is None:                  # uproot(i, k)
                        parents[i] = k
                    l_nz[i] += 1
                    flag[i] = k
                    i = parents[i]
    colptr = [0] * (n + 1)
    prev = 0
    for k in range(n):
        colptr[k] = prev
        prev += l_nz[k]
    colptr[n] = prev
    return parents, l_nz, colptr


def numeric_sequential(n, indptr, indices, data, perm, colptr, parents):
    """ldl_numeric (lib.rs:502-593): (l_indices, l_data, d).  Raises Singular at the first k with d[k] == 0."""
    perm, pinv = _perms(n, perm)
    nnz = colptr[n]
    l_indices, l_data = [0] * nnz, [0.0] * nnz
    diag, y = [0.0] * n, [0.0] * n
    l_nz, flag = [0] * n, [0] * n
    stack = [0] * n                                          # DStack: left grows up from 0, right grows down from n
    for k in range(n):
        flag[k] = k
        y[k] = 0.0
        l_nz[k] = 0
        right_head = n                                       # clear_right
        o = perm[k]
        for p in range(int(indptr[o]), int(indptr[o + 1])):
            inner = pinv[int(indices[p])]
            if inner > k:
                continue
            y[inner] = y[inner] + float(data[p])
            i = inner
            left = 0                                         # clear_left
            while flag[i] != k:
                stack[left] = i                              # push_left
                left += 1
                flag[i] = k
                i = parents[i]
            while left > 0:                                  # push_left_on_right: pop_left, push_right
                left -= 1
                right_head -= 1
                stack[right_head] = stack[left]
        diag[k] = y[k]
        y[k] = 0.0
        for i in stack[right_head:n]:                        # iter_right
            yi = y[i]
            y[i] = 0.0
            p2 = colptr[i] + l_nz[i]
            for q in range(colptr[i], p2):
                y[l_indices[q]] = y[l_indices[q]] - l_data[q] * yi
            l_ki = yi / diag[i]
            diag[k] = diag[k] - l_ki * yi
            l_indices[p2] = k
            l_data[p2] = l_ki
            l_nz[i] += 1
        if diag[k] == 0.0:
            raise Singular(k)
    return l_indices, l_data, diag


def row_patterns(n, indptr, indices, perm, parents):
    """For every row k the entries (i, t) of its pattern: rows are independent given the final parents."""
    perm, pinv = _perms(n, perm)
    rows = []
    for k in range(n):
        first = {}
        o = perm[k]
        for t, p in enumerate(range(int(indptr[o]), int(indptr[o + 1]))):
            i = pinv[int(indices[p])]
            while i < k:
                if i in first and first[i] < t:
                    break                                    # an earlier entry reached this node and everything above it
                first[i] = t
                i = parents[i]
        rows.append(first)
    return rows


def numeric_closed(n, indptr, indices, data, perm, colptr, parents, ascending=False, stop_at_singular=True):
    """The kernels' formulation.  stop_at_singular=False goes on past zero pivots the way the device does (x / 0 in IEEE) and
    returns the smallest singular index as a fourth value."""
    perm_, pinv = _perms(n, perm)
    rows = row_patterns(n, indptr, indices, perm, parents)
    nnz = colptr[n]
    # the column form: rows ascending inside every column
    fill = list(colptr[:n])
    l_indices = [0] * nnz
    slot = {}
    for k in range(n):
        for i in sorted(rows[k]):
            l_indices[fill[i]] = k
            slot[(k, i)] = fill[i]
            fill[i] += 1
    assert fill == list(colptr[1:]), "the parents do not give the column counts"
    l_data = [0.0] * nnz
    diag = [0.0] * n
    singular = None
    with np.errstate(all="ignore"):
        for k in range(n):
            y = dict.fromkeys(rows[k], 0.0)
            dk = 0.0
            o = perm_[k]
            for p in range(int(indptr[o]), int(indptr[o + 1])):
                i = pinv[int(indices[p])]
                if i < k:
                    y[i] = 0.0 + float(data[p])
                elif i == k:
                    dk = 0.0 + float(data[p])
            order = sorted(rows[k]) if ascending else sorted(rows[k], key=lambda i: (-rows[k][i], i))
            for i in order:
                yi = y[i]
                s = slot[(k, i)]
                for q in range(colptr[i], s):
                    y[l_indices[q]] = y[l_indices[q]] - l_data[q] * yi
                l_ki = float(np.float64(yi) / np.float64(diag[i]))
                dk = dk - l_ki * yi
                l_data[s] = l_ki
            diag[k] = dk
            if dk == 0.0:
                if stop_at_singular:
                    raise Singular(k)
                if singular is None:
                    singular = k
    if stop_at_singular:
        return l_indices, l_data, diag
    return l_indices, l_data, diag, singular


def factor(n, indptr, indices, data, perm=None, closed=False):
    """(parents, colptr, l_indices, l_data, d) of LdlNumeric::new_perm without the symmetry check"""
    parents, _, colptr = symbolic(n, indptr, indices, perm)
    f = numeric_closed if closed else numeric_sequential
    l_indices, l_data, d = f(n, indptr, indices, data, perm, colptr, parents)
    return parents, colptr, l_indices, l_data, d


def ldl_lsolve(n, colptr, l_indices, l_data, x):
    """lib.rs:597-609, in place on the list x"""
    for c in range(n):
        xc = x[c]
        for q in range(colptr[c], colptr[c + 1]):
            x[l_indices[q]] -= l_data[q] * xc
    return x


def ldl_ltsolve(n, colptr, l_indices, l_data, x):
    """lib.rs:613-626"""
    for c in range(n - 1, -1, -1):
        xc = x[c]
        for q in range(colptr[c], colptr[c + 1]):
            xc -= l_data[q] * x[l_indices[q]]
        x[c] = xc
    return x


def diag_solve(d, x):
    """linalg.rs:17-29"""
    for i in range(len(x)):
        x[i] = float(np.float64(x[i]) / np.float64(d[i]))
    return x


def solve(n, colptr, l_indices, l_data, d, perm, b):
    """LdlNumeric::solve (lib.rs:403-409): (x, [P b after lsolve, after diag_solve, after ltsolve])"""
    perm, pinv = _perms(n, perm)
    x = [float(b[perm[i]]) for i in range(n)]                # &P * rhs: y[i] = x[p[i]]
    stages = []
    ldl_lsolve(n, colptr, l_indices, l_data, x)
    stages.append(list(x))
    diag_solve(d, x)
    stages.append(list(x))
    ldl_ltsolve(n, colptr, l_indices, l_data, x)
    stages.append(list(x))
    return [x[pinv[i]] for i in range(n)], stages


def bits(values):
    return np.asarray(values, dtype=np.float64).view(np.uint64)


# ---- test matrices -------------------------------------------------------------------------------------------------------

def random_symmetric(n, density, seed, dominant=True):
    """A symmetric matrix in CSR (== its CSC) with a full stored diagonal: off-diagonal values with many mantissa bits, so that
    the order of the subtractions shows; dominant: diagonal > the row's absolute sum (no zero pivots, modest growth)."""
    rng = np.random.RandomState(seed)
    a = np.zeros((n, n))
    mask = np.triu(rng.rand(n, n) < density, 1)
    a[mask] = rng.standard_normal(int(mask.sum())) * 3.0
    a = a + a.T
    diag = rng.rand(n) + 0.5
    if dominant:
        diag = diag + np.abs(a).sum(axis=1)
    a[np.arange(n), np.arange(n)] = diag
    return dense_to_cs(a, keep_diagonal=True)


def dense_to_cs(a, keep_diagonal=False):
    n = a.shape[0]
    indptr, indices, data = [0], [], []
    for r in range(n):
        for c in range(a.shape[1]):
            if a[r, c] != 0.0 or (keep_diagonal and r == c):
                indices.append(c)
                data.append(float(a[r, c]))
        indptr.append(len(indices))
    return n, np.array(indptr, dtype=np.uint64), np.array(indices, dtype=np.uint64), np.array(data, dtype=np.float64)
