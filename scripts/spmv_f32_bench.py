#!/usr/bin/env python3
"""Warm time of the f32 SpMV (sprs_hip_spmv_f32: the nnz-tile plan, its only one) against the f64 SpMV of the same matrix in
the same run: forced onto the plain tile plan (spmv_xcs = 2, which also keeps the banded plan off) — the like-for-like
comparison: same kernel structure, 8 instead of 12 bytes of stream per entry with 4-byte indices — and on its default plan.
Inputs: the 5-point Laplacian of heat.rs on a 4096 x 4096 grid and an R-MAT matrix of 1 M rows, 4-byte indices both.
Every figure is the median of `reps` windows of `inner` SpMVs each, after a warm-up, timed with the host clock around a
device synchronise.  One JSON line per case: stdout and profiles/spmv_f32_bench.jsonl.
usage: spmv_f32_bench.py [reps] [inner]"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sprs_amd                                                      # noqa: E402
from sprs_amd import gen, prod                                       # noqa: E402
from sprs_amd.device import DeviceCsMat, DeviceCsMatF32, DeviceVec, DeviceVecF32   # noqa: E402


def timed(mat, x, y, reps, inner):
    for _ in range(5):                                               # warm-up: plan (the f64 copy plans come with multiply #2), code objects
        prod.csmat_mul_vec(mat, x, out=y)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            prod.csmat_mul_vec(mat, x, out=y)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / inner)
    return statistics.median(ts) * 1e3, min(ts) * 1e3, max(ts) * 1e3


def case(name, n, indptr, indices, data, reps, inner):
    dev = indptr.device
    nnz = int(indices.numel())
    x64 = gen.dense_vector(n, seed=3, device=dev)
    x32, d32 = x64.float(), data.float()
    y64, y32 = torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.float32, device=dev)
    out = {"matrix": name, "n": n, "nnz": nnz, "index_bytes": indices.element_size(), "indptr_bytes": indptr.element_size(),
           "reps": reps, "inner": inner}
    a32 = DeviceCsMatF32.wrap_torch((n, n), indptr, indices, d32).prepare()
    med, lo, hi = timed(a32, DeviceVecF32.borrow(x32), DeviceVecF32.borrow(y32), reps, inner)
    out.update(f32_tile_ms=round(med, 4), f32_tile_min_ms=round(lo, 4), f32_tile_max_ms=round(hi, 4))
    # streamed bytes the algorithm needs: values + indices + indptr + x once + y once
    b32 = nnz * (4 + indices.element_size()) + (n + 1) * indptr.element_size() + 2 * n * 4
    b64 = nnz * (8 + indices.element_size()) + (n + 1) * indptr.element_size() + 2 * n * 8
    out.update(f32_algorithmic_GBps=round(b32 / med / 1e6, 1))
    sprs_amd.set_option("spmv_xcs", 2)                               # plain tile plan: no XCD-sliced, no banded copy
    try:
        a64 = DeviceCsMat.wrap_torch((n, n), indptr, indices, data).prepare()
        med64, lo64, hi64 = timed(a64, DeviceVec.borrow(x64), DeviceVec.borrow(y64), reps, inner)
        assert a64.spmv_plan_info()[0] == 1
    finally:
        sprs_amd.set_option("spmv_xcs", 0)
    out.update(f64_tile_ms=round(med64, 4), f64_tile_min_ms=round(lo64, 4), f64_tile_max_ms=round(hi64, 4),
               f64_tile_algorithmic_GBps=round(b64 / med64 / 1e6, 1), f32_over_f64_tile=round(med / med64, 3))
    a64d = DeviceCsMat.wrap_torch((n, n), indptr, indices, data).prepare()
    medd, lod, hid = timed(a64d, DeviceVec.borrow(x64), DeviceVec.borrow(y64), reps, inner)
    out.update(f64_default_ms=round(medd, 4), f64_default_min_ms=round(lod, 4), f64_default_max_ms=round(hid, 4),
               f64_default_plan_kind=a64d.spmv_plan_info()[0], f32_over_f64_default=round(med / medd, 3))
    # the f32 result against the f64 one of the same inputs, relative to sum |a x| (u = 2^-24 per rounding)
    err = (y32.double() - y64).abs().max().item()
    out.update(max_abs_diff_f32_vs_f64=err)
    return out


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    inner = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    if not torch.cuda.is_available():
        raise SystemExit("spmv_f32_bench.py: no GPU — nothing is measured without one")
    dev = torch.device("cuda", 0)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    lines = []
    g = 4096
    ip, ix, dt = gen.grid_laplacian(g, g, device=dev, idx_dtype=torch.int32, ptr_dtype=torch.int32)
    lines.append(case("5-pt Laplacian %d^2" % g, g * g, ip, ix, dt, reps, inner))
    del ip, ix, dt
    n = 1_000_000
    ip, ix, dt = gen.rmat_csr(n, 16, device=dev, idx_dtype=torch.int32, ptr_dtype=torch.int32)
    lines.append(case("R-MAT 1M x 16", n, ip, ix, dt, reps, inner))
    out_dir = os.environ.get("SPMV_F32_BENCH_OUT", os.path.join(ROOT, "profiles"))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "spmv_f32_bench.jsonl"), "w") as f:
        for line in lines:
            s = json.dumps(line)
            print(s)
            f.write(s + "\n")


if __name__ == "__main__":
    main()
