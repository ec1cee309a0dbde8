#!/usr/bin/env python3
"""Warm time of the f32 SpMM (sprs_hip_csmat_mulacc_dense_f32, operator form, row-major operands) in both lane forms of its
entry-stream kernel (option spmm_f32_pair = 2 / 0) and under the default rule (1: auto) against the f64 SpMM (sprs_hip_csmat_mulacc_dense_f64) of the same matrix
and the same rhs values in the same run.  4-byte indices, option spmm_relayout on auto.
Inputs: an R-MAT matrix of 1 M rows x 16 entries and the 5-point Laplacian on a 2048 x 2048 grid; k = 8, 16, 32, 64.
Every figure is the median / minimum / maximum of `reps` windows of `inner` products each, after a warm-up, timed by HIP events
on the launch stream (the null stream).  One JSON line per (matrix, k, lane form): stdout and profiles/spmm_f32_bench.jsonl;
`f32_le_f64` says whether the f32 median is no slower than the f64 median of the same run, with the f64 windows' own spread
(max - min) as the margin.
usage: spmm_f32_bench.py [reps] [inner]"""
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sprs_amd                                                      # noqa: E402
from sprs_amd import _ffi, gen                                       # noqa: E402
from sprs_amd.device import DeviceCsMat, DeviceCsMatF32             # noqa: E402

KS = (8, 16, 32, 64)


def timed(entry, handle, rhs, out, rows, cols, k, reps, inner):
    """ms per product: (median, min, max) over `reps` windows"""
    def go():
        _ffi.check(entry(handle, C.c_void_p(rhs.data_ptr()), cols, k, _ffi.ROW_MAJOR, k, C.c_void_p(out.data_ptr()), rows, _ffi.ROW_MAJOR, k, 0, None))
    for _ in range(5):                                               # warm-up: the plan, the carry buffers, the code objects
        go()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            go()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / inner)
    return statistics.median(ts), min(ts), max(ts)


def cases(name, n, indptr, indices, data, reps, inner):
    dev = indptr.device
    nnz = int(indices.numel())
    d32 = data.float()
    d64 = d32.double()                                               # the same values in both precisions
    a32 = DeviceCsMatF32.wrap_torch((n, n), indptr, indices, d32)
    a64 = DeviceCsMat.wrap_torch((n, n), indptr, indices, d64)
    lines = []
    for k in KS:
        g = torch.Generator(device=dev).manual_seed(k)
        rhs32 = torch.rand((n, k), generator=g, device=dev, dtype=torch.float32) - 0.5
        rhs64 = rhs32.double()
        out32 = torch.empty((n, k), dtype=torch.float32, device=dev)
        out64 = torch.empty((n, k), dtype=torch.float64, device=dev)
        med64, lo64, hi64 = timed(_ffi.lib.sprs_hip_csmat_mulacc_dense_f64, a64._h, rhs64, out64, n, n, k, reps, inner)
        for pair in (2, 0, 1):                                         # paired wherever eligible, scalar, auto (the default)
            sprs_amd.set_option("spmm_f32_pair", pair)
            try:
                med, lo, hi = timed(_ffi.lib.sprs_hip_csmat_mulacc_dense_f32, a32._h, rhs32, out32, n, n, k, reps, inner)
            finally:
                sprs_amd.set_option("spmm_f32_pair", 1)
            torch.cuda.synchronize()
            # bytes the algorithm needs once: values + indices + indptr + rhs + out
            b32 = nnz * (4 + indices.element_size()) + (n + 1) * indptr.element_size() + 2 * n * k * 4
            b64 = nnz * (8 + indices.element_size()) + (n + 1) * indptr.element_size() + 2 * n * k * 8
            lines.append({
                "matrix": name, "n": n, "nnz": nnz, "k": k, "index_bytes": indices.element_size(), "indptr_bytes": indptr.element_size(),
                "reps": reps, "inner": inner, "spmm_f32_pair": pair,
                "f32_ms": round(med, 4), "f32_min_ms": round(lo, 4), "f32_max_ms": round(hi, 4),
                "f64_ms": round(med64, 4), "f64_min_ms": round(lo64, 4), "f64_max_ms": round(hi64, 4),
                "f32_over_f64": round(med / med64, 3), "f32_le_f64": bool(med <= med64 + (hi64 - lo64)),
                "f32_rhs_rows_per_s": round(nnz / med / 1e6, 2), "f32_algorithmic_GBps": round(b32 / med / 1e6, 1),
                "f64_algorithmic_GBps": round(b64 / med64 / 1e6, 1),
                "max_abs_diff_f32_vs_f64": (out32.double() - out64).abs().max().item(),
            })
            print(json.dumps(lines[-1]), flush=True)
    return lines


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    inner = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    if not torch.cuda.is_available():
        raise SystemExit("spmm_f32_bench.py: no GPU — nothing is measured without one")
    dev = torch.device("cuda", 0)
    lines = []
    n = 1_000_000
    ip, ix, dt = gen.rmat_csr(n, 16, device=dev, idx_dtype=torch.int32, ptr_dtype=torch.int32)
    lines += cases("R-MAT 1M x 16", n, ip, ix, dt, reps, inner)
    del ip, ix, dt
    g = 2048
    ip, ix, dt = gen.grid_laplacian(g, g, device=dev, idx_dtype=torch.int32, ptr_dtype=torch.int32)
    lines += cases("5-pt Laplacian %d^2" % g, g * g, ip, ix, dt, reps, inner)
    out_dir = os.environ.get("SPMM_F32_BENCH_OUT", os.path.join(ROOT, "profiles"))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "spmm_f32_bench.jsonl"), "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
