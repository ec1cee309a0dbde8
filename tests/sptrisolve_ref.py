"""Plain-Python restatement of the reference's sparse-rhs lower triangular solve (lsolve_csc_sparse_rhs,
sprs/src/sparse/linalg/trisolve.rs:286-358, with lspsolve_csc_process_col, :114-149): scalar float64 loops, no vectorised sum
that could reorder.

  reference_order  the function as written: the double-stack depth-first search, the right stack read from its head, the
                   columns processed in that order on a workspace that starts from +0.0
  ascending        the contract of the device twin (include/sprs_hip.h): the same reach as a set, its columns processed in
                   ASCENDING order, fill-in from +0.0, the smallest singular index of the reach reported

Both return (pattern, values): the pattern as a list of indices (reference_order: the right stack's order; ascending: sorted)
and the value of every pattern index, in the same order."""
import numpy as np

from trisolve_ref import Singular


def _lists(ip, ix, dt):
    return [int(v) for v in ip], [int(v) for v in ix], [float(v) for v in dt]


def _process_col(ip, ix, dt, c, x):
    """lspsolve_csc_process_col, trisolve.rs:114-149"""
    diag = None
    for p in range(ip[c], ip[c + 1]):                 # col.get(col_ind)
        if ix[p] == c:
            diag = dt[p]
            break
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


def dfs_pattern(n, ip, ix, rhs_idx):
    """trisolve.rs:322-348: the right stack, read from its head (iter_right)"""
    visited = [False] * n
    right = []
    for root in rhs_idx:
        if visited[root]:
            continue
        left = [("enter", root)]
        while left:
            kind, ind = left.pop()
            if kind == "enter":
                if visited[ind]:
                    continue
                visited[ind] = True
                left.append(("exit", ind))
                for p in range(ip[ind], ip[ind + 1]):
                    left.append(("enter", ix[p]))
            else:
                right.append(ind)                     # push_right: the head moves down ...
    return right[::-1]                                # ... so the last one pushed is read first


def reference_order(n, ip, ix, dt, rhs_idx, rhs_val):
    ip, ix, dt = _lists(ip, ix, dt)
    rhs_idx = [int(v) for v in rhs_idx]
    pattern = dfs_pattern(n, ip, ix, rhs_idx)
    x = [0.0] * n                                     # the workspace (the reference takes whatever the caller passes)
    for i, v in zip(rhs_idx, rhs_val):                # rhs.scatter, trisolve.rs:351
        x[i] = float(v)
    for c in pattern:
        _process_col(ip, ix, dt, c, x)
    return pattern, np.array([x[c] for c in pattern], dtype=np.float64)


def reach(n, ip, ix, rhs_idx):
    """the set the search finds, sorted: the closure of the stored indices of rhs under "every stored entry of a column" """
    ip, ix = [int(v) for v in ip], [int(v) for v in ix]
    seen = set()
    todo = [int(v) for v in rhs_idx]
    while todo:
        c = todo.pop()
        if c in seen:
            continue
        seen.add(c)
        todo.extend(ix[ip[c]:ip[c + 1]])
    return sorted(seen)


def ascending(n, ip, ix, dt, rhs_idx, rhs_val):
    pattern = reach(n, ip, ix, rhs_idx)
    ip, ix, dt = _lists(ip, ix, dt)
    x = [0.0] * n
    for i, v in zip(rhs_idx, rhs_val):
        x[int(i)] = float(v)
    for c in pattern:                                 # (raises at the smallest singular index of the reach, with its own reason)
        _process_col(ip, ix, dt, c, x)
    return pattern, np.array([x[c] for c in pattern], dtype=np.float64)


def csc_arrays(n, rows, cols, vals):
    """sorted CSC arrays (uint64 indptr / indices, float64 data) of the entries (rows[k], cols[k], vals[k]); nothing is
    summed or dropped, so explicit zeros, infs and entries above the diagonal stay"""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    order = np.lexsort((rows, cols))
    ip = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=n))]).astype(np.uint64)
    return ip, rows[order].astype(np.uint64), np.asarray(vals, dtype=np.float64)[order]


def exact_system(n, seed, per_col=3, bands=8):
    """a lower triangular system whose solves are exact in float64: dyadic values, power-of-two diagonals, and every
    stored (r, c) leads from one of `bands` index ranges into a later one, so a chain has at most `bands` unknowns"""
    rng = np.random.default_rng(seed)
    band = np.arange(n) * bands // n
    rows, cols = list(range(n)), list(range(n))
    vals = list(rng.choice([1.0, -1.0, 2.0, -2.0, 0.5, 4.0], n))
    for c in range(n):
        later = np.flatnonzero(band > band[c])
        if later.size:
            for r in rng.choice(later, min(per_col, later.size), replace=False):
                rows.append(int(r))
                cols.append(c)
                vals.append(float(rng.choice([1.0, -1.0, 2.0, -2.0, 0.5, -0.5, 0.25])))
    return csc_arrays(n, rows, cols, vals)


def depth(n, ip, ix, rhs_idx):
    """breadth-first levels of the search from the stored indices of rhs: the frontiers that are not empty"""
    ip, ix = [int(v) for v in ip], [int(v) for v in ix]
    seen = set(int(v) for v in rhs_idx)
    front, levels = sorted(seen), 0
    while front:
        levels += 1
        nxt = []
        for c in front:
            for p in range(ip[c], ip[c + 1]):
                if ix[p] not in seen:
                    seen.add(ix[p])
                    nxt.append(ix[p])
        front = nxt
    return levels
