#!/usr/bin/env python3
"""The four device triangular solves (twins of sprs::linalg::trisolve, sprs/src/sparse/linalg/trisolve.rs) on the lower and
upper parts of the heat system of a G x G grid and of a random strictly diagonally dominant system: levels, ms per solve, us
per level, the one-time cost of the first call (level order; for CSC handles also the CSR form), the scaled residual of the
solution, and — the yardstick — one Gauss-Seidel sweep (max_iter = 1: sweep + residual SpMV + convergence scalar) on the handle
that lsolve_csr ran on, in the same run.  One JSON line per solve.
usage: trisolve_bench.py [G ...]     (default 4096 -4000000; G < 0: the random system of -G rows of scripts/gauss_seidel_bench.py)"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sprs_amd import _ffi, linalg                             # noqa: E402
from sprs_amd.device import CSC, CSR, DeviceCsMat, DeviceVec  # noqa: E402
from oracle import oracle                                     # noqa: E402  (the grid generator, nothing else)

REPEATS = 5


def system(g):
    if g > 0:
        shape, ip, ix, dt = oracle.grid_laplacian(g, g)
        return "heat %d x %d" % (g, g), sp.csr_matrix((dt, ix.astype(np.int64), ip.astype(np.int64)), shape=shape)
    n = -g
    rng = np.random.default_rng(1)
    r = np.repeat(np.arange(n), 8)
    c = rng.integers(0, n, size=8 * n)
    m = sp.coo_matrix((rng.standard_normal(8 * n), (r, c)), shape=(n, n)).tocsr()
    m = (m + sp.diags(np.abs(m).sum(axis=1).A1 + 1.0)).tocsr()
    return "random %d rows, 8 per row" % n, m


def restore(x, b):
    _ffi.check(_ffi.lib.sprs_hip_memcpy_d2d(C.c_void_p(x.ptr), C.c_void_p(b.ptr), x.n * 8, None))
    _ffi.check(_ffi.lib.sprs_hip_synchronize(None))


def main():
    for g in [int(v) for v in sys.argv[1:]] or [4096, -4000000]:
        name, full = system(g)
        n = full.shape[0]
        b = np.random.default_rng(2).standard_normal(n)
        d_b = DeviceVec.from_host(b)
        x = DeviceVec(n)
        for uplo, part in (("l", sp.tril(full).tocsr()), ("u", sp.triu(full).tocsr())):
            part.sort_indices()
            for storage in ("csr", "csc"):
                kind = uplo + "solve_" + storage
                m = part.tocsc() if storage == "csc" else part
                m.sort_indices()
                a = DeviceCsMat.from_host((n, n), m.indptr.astype(np.uint64), m.indices.astype(np.uint64), m.data,
                                          storage=CSC if storage == "csc" else CSR, validate=False)
                fn = getattr(linalg, kind + "_dense_rhs")
                restore(x, d_b)
                t0 = time.perf_counter()
                res = fn(a, x)
                first = time.perf_counter() - t0
                got = x.to_host()
                resid = float(np.abs(part @ got - b).max() / max(np.abs(b).max(), 1e-300))
                times = []
                for _ in range(REPEATS):
                    restore(x, d_b)
                    t0 = time.perf_counter()
                    fn(a, x)
                    times.append(time.perf_counter() - t0)
                same = bool(np.array_equal(x.to_host(), got))
                per = float(np.median(times))
                line = {"system": name, "solve": kind, "rows": n, "nnz": int(m.nnz), "levels": res.levels,
                        "ms_per_solve": round(per * 1e3, 3), "us_per_level": round(per * 1e6 / max(res.levels, 1), 3),
                        "ms_min_max": [round(min(times) * 1e3, 3), round(max(times) * 1e3, 3)], "repeats": REPEATS,
                        "first_call_s_plans_included": round(first, 3), "max_residual_over_max_b": resid, "repeatable_bits": same}
                if kind == "lsolve_csr":                       # the yardstick: one sweep on the same handle, the same level order
                    rhs = DeviceVec.from_host(b)
                    linalg.gauss_seidel(a, x, rhs, 1, -1.0)    # warm: the SpMV plan of the residual
                    gs = []
                    for _ in range(REPEATS):
                        restore(x, d_b)
                        t0 = time.perf_counter()
                        r = linalg.gauss_seidel(a, x, rhs, 1, -1.0)
                        gs.append(time.perf_counter() - t0)
                    line["gauss_seidel_one_sweep_with_residual_ms"] = round(float(np.median(gs)) * 1e3, 3)
                    line["gauss_seidel_us_per_level"] = round(float(np.median(gs)) * 1e6 / max(r.levels, 1), 3)
                print(json.dumps(line), flush=True)
                del a, m
            del part


if __name__ == "__main__":
    main()
