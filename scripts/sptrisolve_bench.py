#!/usr/bin/env python3
"""The device sparse-rhs lower triangular solve (twin of lsolve_csc_sparse_rhs, sprs/src/sparse/linalg/trisolve.rs:286-358) on
  * L = the lower triangle of the 5-point Laplacian of a G x G grid (the heat example's matrix), and
  * the lower triangle of an R-MAT matrix with a dominant diagonal,
each with unit right-hand sides whose reach is about 0.01 %, 1 % and 100 % of n (the nearest the matrix offers: the roots are
picked on the host by a breadth-first search over the columns).  Per case: |reach|, the levels and launches of the reach, the
median time of the solve, and — the yardstick — the median time of lsolve_csc_dense_rhs on the same handle in the same run
(its right-hand side restored by a device copy outside the timed region).  One JSON line per case.
usage: sptrisolve_bench.py [G [rmat_rows]]     (default 1024 1048576)"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import breadth_first_order

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sprs_amd import _ffi, gen, linalg                            # noqa: E402
from sprs_amd.device import CSC, DeviceCsMat, DeviceCsVec, DeviceVec  # noqa: E402

REPEATS = 7
TARGETS = (1e-4, 1e-2, 1.0)


def lower_of(indptr, indices, data, n):
    a = sp.csr_matrix((data.numpy(), indices.numpy().astype(np.int64), indptr.numpy().astype(np.int64)), shape=(n, n))
    low = sp.tril(a, -1).tocsr()
    low = (low + sp.diags(np.abs(low).sum(axis=1).A1 + 1.0)).tocsc()      # every diagonal stored and dominant
    low.sort_indices()
    return low


def reach_size(graph, root):
    return int(breadth_first_order(graph, root, directed=True, return_predecessors=False).size)


def pick_roots(low, candidates):
    """for every target share of n, the candidate root whose reach comes nearest"""
    n = low.shape[0]
    graph = sp.csr_matrix(low.T)                                          # edge c -> r for every stored (r, c)
    sizes = {int(c): reach_size(graph, int(c)) for c in candidates}
    return [min(sizes, key=lambda c: abs(np.log(sizes[c] / (t * n)))) for t in TARGETS]


def restore(x, b):
    _ffi.check(_ffi.lib.sprs_hip_memcpy_d2d(C.c_void_p(x.ptr), C.c_void_p(b.ptr), x.n * 8, None))
    _ffi.check(_ffi.lib.sprs_hip_synchronize(None))


def run(name, low, roots):
    n = low.shape[0]
    a = DeviceCsMat.from_host((n, n), low.indptr.astype(np.uint64), low.indices.astype(np.uint64), low.data, storage=CSC, validate=False)
    x = DeviceVec(n)
    for root in roots:
        rhs = DeviceCsVec.from_host(n, np.array([root], dtype=np.uint64), np.ones(1))
        d_b = rhs.to_dense()
        t0 = time.perf_counter()
        out = linalg.lsolve_csc_sparse_rhs(a, rhs)
        first = time.perf_counter() - t0
        restore(x, d_b)
        linalg.lsolve_csc_dense_rhs(a, x)                                 # warm; also the check: the same solution
        _, oi, ov = out.to_host()
        dense = x.to_host()
        err = float(np.abs(dense[oi.astype(np.int64)] - ov).max())
        outside = np.ones(n, dtype=bool)
        outside[oi.astype(np.int64)] = False
        sparse_t, dense_t = [], []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            out = linalg.lsolve_csc_sparse_rhs(a, rhs)
            sparse_t.append(time.perf_counter() - t0)
            restore(x, d_b)
            t0 = time.perf_counter()
            res = linalg.lsolve_csc_dense_rhs(a, x)
            dense_t.append(time.perf_counter() - t0)
        print(json.dumps({"system": name, "rows": n, "nnz": int(low.nnz), "root": int(root), "reach": out.reach,
                          "reach_share": round(out.reach / n, 6), "reach_levels": out.reach_levels, "reach_launches": out.reach_launches,
                          "sparse_rhs_ms": round(float(np.median(sparse_t)) * 1e3, 3),
                          "sparse_rhs_ms_min_max": [round(min(sparse_t) * 1e3, 3), round(max(sparse_t) * 1e3, 3)],
                          "dense_rhs_ms": round(float(np.median(dense_t)) * 1e3, 3), "dense_levels": res.levels, "repeats": REPEATS,
                          "first_call_s_plans_included": round(first, 3), "max_abs_difference_from_the_dense_solve": err,
                          "dense_solve_is_zero_outside_the_reach": bool(not dense[outside].any())}), flush=True)


def main():
    g = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    rows = int(sys.argv[2]) if len(sys.argv) > 2 else 1 << 20
    low = lower_of(*gen.grid_laplacian(g, g), g * g)
    diag = [(g - 1 - k) * g + (g - 1 - k) for k in (2, 5, 8, 11, 14, 20, 50, 90, 100, 110, 130, g // 2, g - 2) if 0 < k < g - 1]
    run("heat %d x %d, lower triangle" % (g, g), low, pick_roots(low, diag))
    low = lower_of(*gen.rmat_csr(rows, 8), rows)
    rng = np.random.default_rng(1)
    cand = np.unique(np.concatenate([np.arange(8), rng.integers(0, rows, 48), rows - 1 - rng.integers(0, rows // 50, 24)]))
    run("R-MAT %d rows, 8 per row, lower triangle" % rows, low, pick_roots(low, cand))


if __name__ == "__main__":
    main()
