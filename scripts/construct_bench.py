#!/usr/bin/env python3
"""Construction timing (sprs_hip_csmat_kronecker_f64, sprs_hip_csmat_vstack, sprs_hip_csmat_bmat; sprs_amd/csrc/construct.hpp):
  kron(I_n, T_n), kron(T_n, I_n)   the two halves of the grid Laplacian, T_n tridiagonal, 8-byte indices and indptr
  kron(R, R')                      two R-MAT matrices of 2^12 rows: hub row (x) hub row
  vstack                           the 8-way slice_outer cut of an R-MAT matrix (default 1M rows), put back together
  bmat                             the 2 x 2 saddle point [[A, B^T], [B, None]], A a grid Laplacian, B a quarter as many rows
The yardstick of each case is a device-to-device copy of the RESULT's bytes (sprs_hip_memcpy_d2d of its three arrays), timed in
the same run: the copy reads and writes them, the Kronecker product only writes them (its operands stay in cache), the stackers
read and write once.  Warm, timed with events on the null stream, median of `reps` runs; the calls include the allocation of
the result (from the pool once warm).  One JSON line per case.
usage: construct_bench.py [--n N] [--rmat-log2 K] [--rmat-per-row D] [--stack-n N] [--grid G] [--reps R]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sprs_amd                                       # noqa: E402
from sprs_amd import _ffi, construct, gen             # noqa: E402
from sprs_amd.device import DeviceCsMat               # noqa: E402


def median_ms(call, reps):
    """the calls block until their result is complete on the null stream; events bracket each one"""
    for _ in range(2):
        call()
    out = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        call()
        t1.record()
        t1.synchronize()
        out.append(t0.elapsed_time(t1))
    return float(np.median(out))


def result_bytes(res):
    r, c, nnz, pb, ib, st = res._info()
    outer = r if st == _ffi.CSR else c
    return (outer + 1) * pb, nnz * ib, nnz * 8


def copy_ms(res, reps):
    """the yardstick: the result's three arrays copied device to device"""
    ip, ix, dt = C.c_void_p(), C.c_void_p(), C.c_void_p()
    _ffi.check(_ffi.lib.sprs_hip_csmat_device_ptrs(res._h, C.byref(ip), C.byref(ix), C.byref(dt)))
    sizes = result_bytes(res)
    dst = [torch.empty(max(s, 8), dtype=torch.uint8, device="cuda") for s in sizes]

    def call():
        for d, src, s in zip(dst, (ip, ix, dt), sizes):
            if s:
                _ffi.check(_ffi.lib.sprs_hip_memcpy_d2d(C.c_void_p(d.data_ptr()), src, s, None))
        _ffi.check(_ffi.lib.sprs_hip_synchronize(None))
    return median_ms(call, reps)


def report(name, call, reps, extra=None):
    res = call()
    nbytes = sum(result_bytes(res))
    ms_copy = copy_ms(res, reps)
    shape, nnz = res.shape(), res.nnz()
    del res
    ms = median_ms(call, reps)
    row = {"case": name, "shape": list(shape), "nnz": nnz, "result_bytes": nbytes, "ms": round(ms, 3), "written_GBs": round(nbytes / ms / 1e6, 1),
           "copy_ms": round(ms_copy, 3), "copy_GBs_each_way": round(nbytes / ms_copy / 1e6, 1), "ratio_to_copy": round(ms / ms_copy, 3)}
    row.update(extra or {})
    print(json.dumps(row), flush=True)
    torch.cuda.empty_cache()
    sprs_amd.pool_trim()


def tridiag(n, idx, ptr):
    lens = np.full(n, 3)
    lens[[0, -1]] = 2
    ip = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=ip[1:])
    rows = np.repeat(np.arange(n), lens)
    off = np.arange(ip[-1]) - ip[rows] - (rows > 0)
    ix = rows + off
    return DeviceCsMat.from_host((n, n), ip.astype(ptr), ix.astype(idx), np.where(ix == rows, 2.0, -1.0))


def wrap(n, cols, arrs):
    ip, ix, dt = arrs
    return DeviceCsMat.wrap_torch((n, cols), ip, ix.to(torch.int32), dt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--rmat-log2", type=int, default=12)
    ap.add_argument("--rmat-per-row", type=float, default=4)
    ap.add_argument("--stack-n", type=int, default=1_000_000)
    ap.add_argument("--grid", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)

    n = args.n
    t, eye = tridiag(n, np.uint64, np.uint64), DeviceCsMat.eye(n)
    report("kron(I_%d, T_%d)" % (n, n), lambda: construct.kronecker_product(eye, t), args.reps)
    report("kron(T_%d, I_%d)" % (n, n), lambda: construct.kronecker_product(t, eye), args.reps)
    del t, eye

    m = 1 << args.rmat_log2
    r1 = wrap(m, m, gen.rmat_csr(m, args.rmat_per_row, seed=1, value_seed=2, device=dev))
    r2 = wrap(m, m, gen.rmat_csr(m, args.rmat_per_row, seed=3, value_seed=4, device=dev))
    longest = [int((x.to_host()[1][1:] - x.to_host()[1][:-1]).max()) for x in (r1, r2)]
    report("kron(rmat 2^%d, rmat 2^%d)" % (args.rmat_log2, args.rmat_log2), lambda: construct.kronecker_product(r1, r2), args.reps,
           {"longest_rows": longest})
    del r1, r2

    sn = args.stack_n
    big = wrap(sn, sn, gen.rmat_csr(sn, 16, seed=5, value_seed=6, device=dev))
    cuts = [sn * k // 8 for k in range(9)]
    parts = [big.slice_outer(s, e) for s, e in zip(cuts[:-1], cuts[1:])]
    report("vstack(8 cuts of rmat n=%d)" % sn, lambda: construct.vstack(parts), args.reps)
    del big, parts

    g = args.grid
    a = wrap(g * g, g * g, gen.grid_laplacian(g, g, device=dev))
    mb = g * g // 4
    b = wrap(g * g, g * g, gen.rmat_csr(g * g, 4, seed=7, value_seed=8, device=dev)).slice_outer(0, mb)
    bt = b.transpose_view().to_other_storage()          # B^T as CSR: the assembly is timed, not a conversion
    report("bmat([[A, Bt], [B, None]]) A = laplacian %d^2" % g, lambda: construct.bmat([[a, bt], [b, None]]), args.reps)


if __name__ == "__main__":
    main()
