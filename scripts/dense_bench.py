#!/usr/bin/env python3
"""Dense <-> sparse timing (sprs_hip_csmat_from_dense_f64, _assign_to_dense_f64, _to_dense_f64, _binop_dense_f64, _add_dense_f64;
sprs_amd/csrc/dense.hpp) on an n x n row-major f64 operand (default n = 16384: 2 GiB) with a fraction `keep` of its elements
above epsilon (default 1 % and 50 %), CSR with 4-byte indices and 8-byte indptr.
The yardstick is a device-to-device copy of the SAME dense buffer (sprs_hip_memcpy_d2d), timed in the same run: it reads the
n * n * 8 bytes once and writes them once.  Against it
  from_dense      reads the operand twice (count pass, emit pass) and writes the entries
  assign_to_dense writes the stored entries only
  to_dense        writes the operand once, then the entries
  binop / add     read the operand once and write it once, then read and write the stored positions
Warm, timed with events on the null stream, median of `reps` runs; from_dense includes the allocation of its result (from the
pool once warm).  One JSON line per entry and fraction.
usage: dense_bench.py [--n N] [--keep F [F ...]] [--reps R]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sprs_amd                                       # noqa: E402
from sprs_amd import _ffi, binop, to_dense            # noqa: E402
from sprs_amd.device import DeviceCsMat, DeviceVec    # noqa: E402
from sprs_amd.prod import DeviceMat                   # noqa: E402


def median_ms(call, reps):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--keep", type=float, nargs="+", default=[0.01, 0.5])
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, nbytes = args.n, args.n * args.n * 8
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    u = torch.rand(n * n, dtype=torch.float64, device=dev, generator=gen)      # uniform in [0, 1): |x| > 1 - keep is kept
    rhs_t = torch.rand(n * n, dtype=torch.float64, device=dev, generator=gen)
    out_t = torch.empty(n * n, dtype=torch.float64, device=dev)
    m = DeviceMat(n, n, DeviceVec.borrow(u))
    rhs = DeviceMat(n, n, DeviceVec.borrow(rhs_t))
    out = DeviceMat(n, n, DeviceVec.borrow(out_t))
    torch.cuda.synchronize()

    def copy():
        _ffi.check(_ffi.lib.sprs_hip_memcpy_d2d(C.c_void_p(out_t.data_ptr()), C.c_void_p(u.data_ptr()), nbytes, None))
        _ffi.check(_ffi.lib.sprs_hip_synchronize(None))
    ms_copy = median_ms(copy, args.reps)
    print(json.dumps({"case": "copy_d2d", "n": n, "bytes": nbytes, "ms": round(ms_copy, 3), "GBs_each_way": round(nbytes / ms_copy / 1e6, 1)}),
          flush=True)

    def sync(f):
        def call():
            f()
            _ffi.check(_ffi.lib.sprs_hip_synchronize(None))
        return call

    for keep in args.keep:
        eps = 1.0 - keep
        a = DeviceCsMat.csr_from_dense(m, eps, np.uint32, np.uint64)
        nnz = a.nnz()
        cases = [
            ("from_dense", lambda: DeviceCsMat.csr_from_dense(m, eps, np.uint32, np.uint64), 2 * nbytes + nnz * 12),
            ("assign_to_dense", sync(lambda: to_dense.assign_to_dense(out, a)), nnz * 20),
            ("to_dense", sync(lambda: to_dense.to_dense(a, out)), nbytes + nnz * 20),
            ("binop_dense add 2.5 -0.5", sync(lambda: binop.csmat_binop_dense_raw(a, rhs, binop.ADD, out, 2.5, -0.5)), 2 * nbytes + nnz * 28),
            ("binop_dense mul 2.5", sync(lambda: binop.csmat_binop_dense_raw(a, rhs, binop.MUL, out, 2.5)), 2 * nbytes + nnz * 28),
            ("add_dense (&A + &D)", sync(lambda: _ffi.check(_ffi.lib.sprs_hip_csmat_add_dense_f64(
                a._h, C.c_void_p(rhs_t.data_ptr()), n, n, _ffi.ROW_MAJOR, n, C.c_void_p(out_t.data_ptr()), None))), 2 * nbytes + nnz * 28),
        ]
        for name, call, moved in cases:
            ms = median_ms(call, args.reps)
            print(json.dumps({"case": name, "n": n, "keep": keep, "nnz": nnz, "ms": round(ms, 3), "bytes_moved": moved,
                              "GBs": round(moved / ms / 1e6, 1), "copy_ms": round(ms_copy, 3), "ratio_to_copy": round(ms / ms_copy, 3)}),
                  flush=True)
        del a
        sprs_amd.pool_trim()


if __name__ == "__main__":
    main()
