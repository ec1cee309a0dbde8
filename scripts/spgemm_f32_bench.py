#!/usr/bin/env python3
"""Warm time of the f32 SpGEMM against the f64 SpGEMM of the same structure and the same (f32-representable) values, in the
same process run, on the two SpGEMM shapes bench.py uses:
  uniform   (2.5 M x 2.5 M) * (2.5 M x 2.5 M), uniform density 4 / cols: every row a lane-group row (sprs-benches' own shape)
  config5   A * A, R-MAT 1 M x 1 M, ~8 entries per row: hash, wave-per-row and workgroup rows, 5.5e9 products
For each shape and precision: (a) the whole product (smmp.mul_csr_csr: counting pass, scans, numeric pass, result allocation
from the block pool) and (b) numeric() on a kept plan into an existing structure (value kernels and the per-call packing of
B's records only).  f64 and f32 ALTERNATE inside every repetition, so that whatever else the machine does hits both; every
figure is the median / minimum / maximum of `reps` repetitions (default 11) after two warm-up rounds, timed by HIP events on the
null stream.  One JSON line per (shape, measure): stdout and profiles/spgemm_f32_bench.jsonl.  `f32_le_f64` says whether
the f32 median is no slower than the f64 median of the same run, with the f64 repetitions' own spread (max - min) as the margin.
8-byte indices and indptr, default options; the f32 probe's verdict travels with every line.
usage: spgemm_f32_bench.py [reps] [shape ...]"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sprs_amd                                                      # noqa: E402
from sprs_amd import gen, smmp                                       # noqa: E402
from sprs_amd.device import DeviceCsMat, DeviceCsMatF32             # noqa: E402


def operands(shape, dev):
    """-> (n, (indptr, indices, f64 values) of A, the same of B or None for A * A)"""
    if shape == "uniform":
        n = 2_500_000
        return n, gen.uniform_csr((n, n), 4.0 / n, seed=11, value_seed=12, device=dev), \
            gen.uniform_csr((n, n), 4.0 / n, seed=21, value_seed=22, device=dev)
    n = 1_000_000
    return n, gen.rmat_csr(n, 8, device=dev, idx_dtype=torch.int64, ptr_dtype=torch.int64, oversample=1.0), None


def timed_pair(run64, run32, reps):
    """ms per call, f64 and f32 alternating: ((median, min, max) f64, the same f32)"""
    t64, t32 = [], []
    for r in range(reps + 2):
        for run, ts in ((run64, t64), (run32, t32)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            if r >= 2:                                               # two warm-up rounds: code objects, pool blocks, the probes
                ts.append(e0.elapsed_time(e1))
    return tuple((statistics.median(t), min(t), max(t)) for t in (t64, t32))


def line(shape, measure, n, nnz_c, reps, f64, f32):
    spread = f64[2] - f64[1]
    return {"shape": shape, "measure": measure, "n": n, "nnz_c": nnz_c, "reps": reps, "index_bytes": 8, "indptr_bytes": 8,
            "f64_ms": round(f64[0], 3), "f64_min_ms": round(f64[1], 3), "f64_max_ms": round(f64[2], 3),
            "f32_ms": round(f32[0], 3), "f32_min_ms": round(f32[1], 3), "f32_max_ms": round(f32[2], 3),
            "f32_over_f64": round(f32[0] / f64[0], 3), "f32_le_f64": bool(f32[0] <= f64[0] + spread)}


def bench(shape, reps, dev):
    n, (a_ip, a_ix, a_dt), b = operands(shape, dev)
    a32v = a_dt.float()
    a64 = DeviceCsMat.wrap_torch((n, n), a_ip, a_ix, a32v.double())       # the same values in both precisions
    a32 = DeviceCsMatF32.wrap_torch((n, n), a_ip, a_ix, a32v)
    if b is None:
        b64, b32 = a64, a32
    else:
        b32v = b[2].float()
        b64 = DeviceCsMat.wrap_torch((n, n), b[0], b[1], b32v.double())
        b32 = DeviceCsMatF32.wrap_torch((n, n), b[0], b[1], b32v)
    keep = {}

    def whole(x, y, tag):
        def go():
            keep[tag] = None                                          # the previous result goes back to the block pool
            keep[tag] = smmp.mul_csr_csr(x, y)
        return go

    out = []
    f64, f32 = timed_pair(whole(a64, b64, 64), whole(a32, b32, 32), reps)
    nnz_c = keep[32].nnz()
    assert nnz_c == keep[64].nnz()
    out.append(line(shape, "whole product", n, nnz_c, reps, f64, f32))
    keep.clear()
    p64, p32 = smmp.SpgemmPlan(a64, b64), smmp.SpgemmPlan(a32, b32)
    c64, c32 = p64.structure(), p32.structure()
    f64, f32 = timed_pair(lambda: p64.numeric(c64), lambda: p32.numeric(c32), reps)
    out.append(line(shape, "kept-plan numeric", n, nnz_c, reps, f64, f32))
    del p64, p32, c64, c32
    return out


def main():
    args = sys.argv[1:]
    reps = int(args[0]) if args and args[0].isdigit() else 11
    shapes = [a for a in args if not a.isdigit()] or ["uniform", "config5"]
    if sprs_amd.device_count() < 1:
        sys.exit("no HIP device: nothing is measured without one")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "spgemm_f32_bench.jsonl"), "a") as f:
        for shape in shapes:
            for ln in bench(shape, reps, dev):
                ln["device"] = torch.cuda.get_device_name(0)
                ln["spgemm_f32_lds_add"] = sprs_amd.get_option("spgemm_f32_lds_add")     # 3: lane order holds and subnormals are kept
                s = json.dumps(ln)
                print(s, flush=True)
                f.write(s + "\n")
            torch.cuda.empty_cache()
            sprs_amd._ffi.check(sprs_amd._ffi.lib.sprs_hip_pool_trim(None))


if __name__ == "__main__":
    main()
