#!/usr/bin/env python3
"""f32 against f64, warm, in the same run, on the same structure: the lower and the upper triangular solve (CSR) on the two
triangles of the 5-point Laplacian of a G x G grid, and one Gauss-Seidel sweep with its residual on the heat system of the
same grid (scripts/trisolve_bench.py and scripts/gauss_seidel_bench.py measure the f64 side alone).  The f32 handle holds the
same values rounded to f32 over the same index widths; the right-hand side is the same numbers rounded to f32.  The solves are bound by the chain of levels —
one publish -> poll hop each — so what the pair of numbers shows is the hop through a 4-byte hand-off word against the hop
through an 8-byte one.  One JSON line per operation, then a line that says which precision was faster.
usage: trisolve_f32_bench.py [G]     (default 1024)"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sprs_amd import _ffi, linalg                                                       # noqa: E402
from sprs_amd.device import DeviceCsMat, DeviceCsMatF32, DeviceVec, DeviceVecF32        # noqa: E402
from oracle import oracle                                                               # noqa: E402  (the grid generator, nothing else)

REPEATS = 9


def restore(x, b, itemsize):
    _ffi.check(_ffi.lib.sprs_hip_memcpy_d2d(C.c_void_p(x.ptr), C.c_void_p(b.ptr), x.n * itemsize, None))
    _ffi.check(_ffi.lib.sprs_hip_synchronize(None))


def timed(call, x, x0, itemsize):
    """median, min and max of REPEATS warm calls, x restored before each; the result of the last one"""
    restore(x, x0, itemsize)
    res = call()                                                   # warm: level plans, the SpMV plan of the residual
    first = x.to_host()
    times = []
    for _ in range(REPEATS):
        restore(x, x0, itemsize)
        t0 = time.perf_counter()
        res = call()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), min(times), max(times), res, bool(np.array_equal(x.to_host(), first, equal_nan=True))


def pair(name, m, b, call_of):
    """one operation in both precisions on the CSR matrix m: call_of(handle, x, rhs) -> the timed call"""
    n = m.shape[0]
    a64 = DeviceCsMat.from_host((n, n), m.indptr.astype(np.uint64), m.indices.astype(np.uint32), m.data, validate=False)
    a32 = DeviceCsMatF32.from_host((n, n), m.indptr.astype(np.uint64), m.indices.astype(np.uint32), m.data.astype(np.float32), validate=False)
    out = {}
    for tag, a, vec, dtype, size in (("f64", a64, DeviceVec, np.float64, 8), ("f32", a32, DeviceVecF32, np.float32, 4)):
        x0 = vec.from_host(b.astype(dtype))
        x = vec(n)
        med, lo, hi, res, same = timed(call_of(a, x, x0), x, x0, size)
        out[tag] = med
        print(json.dumps({"operation": name, "precision": tag, "rows": n, "nnz": int(m.nnz), "levels": res.levels,
                          "ms": round(med * 1e3, 3), "us_per_level": round(med * 1e6 / max(res.levels, 1), 3),
                          "ms_min_max": [round(lo * 1e3, 3), round(hi * 1e3, 3)], "repeats": REPEATS, "repeatable_bits": same}),
              flush=True)
    return out


def main():
    g = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    shape, ip, ix, dt = oracle.grid_laplacian(g, g)
    full = sp.csr_matrix((dt, ix.astype(np.int64), ip.astype(np.int64)), shape=shape)
    n = shape[0]
    b = np.random.default_rng(2).standard_normal(n)
    results = {}
    for uplo, part in (("l", sp.tril(full).tocsr()), ("u", sp.triu(full).tocsr())):
        part.sort_indices()
        fn = getattr(linalg, uplo + "solve_csr_dense_rhs")
        results[uplo + "solve_csr"] = pair("%ssolve_csr, 5-point Laplacian %d x %d" % (uplo, g, g), part,
                                           b, lambda a, x, x0, fn=fn: (lambda: fn(a, x)))
    i, j = np.meshgrid(np.arange(g), np.arange(g), indexing="ij")
    border = (i == 0) | (i == g - 1) | (j == 0) | (j == g - 1)
    rhs = np.where(border, (i + j).astype(np.float64), 0.0).reshape(-1)
    full.sort_indices()

    def sweep_of(a, x, x0):
        d_rhs = type(x).from_host(rhs.astype(x._dtype))
        return lambda: linalg.gauss_seidel(a, x, d_rhs, 1, -1.0)

    results["gauss_seidel"] = pair("gauss_seidel, one sweep with its residual, heat system %d x %d" % (g, g), full, np.zeros(n), sweep_of)
    for name, r in results.items():
        print(json.dumps({"operation": name, "f32_ms": round(r["f32"] * 1e3, 3), "f64_ms": round(r["f64"] * 1e3, 3),
                          "f32_over_f64": round(r["f32"] / r["f64"], 3), "faster": "f32" if r["f32"] < r["f64"] else "f64"}), flush=True)


if __name__ == "__main__":
    main()
