#!/usr/bin/env python3
"""Warm time of the f32 SpMV (sprs_hip_spmv_f32) on each of its plans against the f64 SpMV of the same matrix in the same run.
Per matrix, one JSON line with, for every variant, the median / min / max time of an SpMV, the plan kind (1 nnz tiles, 3 banded),
plan_bytes and the time prepare() took to build the plan:
    f32_tile     the nnz-tile plan (spmv_band = 2)
    f32_auto     default options: what a caller gets (the 5-point Laplacian must stay on kind 1: its rows are shorter than the split)
    f32_band16k  the banded plan forced (spmv_band = 1) with slices of 16384 labels
    f32_band32k  ... of 32768 labels
    f64_tile     the f64 SpMV forced onto the plain tile plan (spmv_xcs = 2, which also keeps the banded plan off)
    f64_default  the f64 SpMV on its default plan (banded on the R-MAT matrices)
A library without the f32 banded plan (the parent commit's, for the A/B below) reports f32_tile and the f64 variants only.
Inputs, 4-byte indices: the 5-point Laplacian of heat.rs on a 4096 x 4096 grid, R-MAT 1 M x 16 and R-MAT 10 M x 16.
Every figure is the median of `reps` windows of `inner` SpMVs each, after a warm-up, timed with the host clock around a
device synchronise.  Lines go to stdout and to profiles/spmv_f32_bench.jsonl.

usage: spmv_f32_bench.py [reps] [inner] [--matrices lap,rmat1m,rmat10m]
       spmv_f32_bench.py [reps] [inner] [--matrices ...] --ab PARENT_TREE RUNS
--ab: boxes differ by several per cent and drift, so the comparison with the parent commit alternates the two in ONE session, one
process per run: RUNS times (PARENT_TREE/scripts/spmv_f32_bench.py — a copy of this file put there —, then this one); every run's
lines and, per matrix and variant, median and range over the runs go to profiles/spmv_f32_band_ab.txt."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATRICES = ("lap", "rmat1m", "rmat10m")


def timed(prod, torch, mat, x, y, reps, inner):
    for _ in range(5):                                               # warm-up: per-stream scratch, code objects
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


def measure(name, n, indptr, indices, data, reps, inner):
    import torch
    import sprs_amd
    from sprs_amd import gen, prod
    from sprs_amd.device import DeviceCsMat, DeviceCsMatF32, DeviceVec, DeviceVecF32
    dev = indptr.device
    nnz = int(indices.numel())
    x64 = gen.dense_vector(n, seed=3, device=dev)
    x32, d32 = x64.float(), data.float()
    y64, y32 = torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.float32, device=dev)
    out = {"matrix": name, "n": n, "nnz": nnz, "index_bytes": indices.element_size(), "indptr_bytes": indptr.element_size(),
           "reps": reps, "inner": inner}
    has_band = hasattr(DeviceCsMatF32, "spmv_plan_info")

    def variant(tag, opts, f32):
        for k, v in opts.items():
            sprs_amd.set_option(k, v)
        try:
            cls, xs, ys = (DeviceCsMatF32, DeviceVecF32.borrow(x32), DeviceVecF32.borrow(y32)) if f32 else (DeviceCsMat, DeviceVec.borrow(x64), DeviceVec.borrow(y64))
            a = cls.wrap_torch((n, n), indptr, indices, d32 if f32 else data)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.prepare()
            torch.cuda.synchronize()
            build = time.perf_counter() - t0
            med, lo, hi = timed(prod, torch, a, xs, ys, reps, inner)
            kind, nbytes = a.spmv_plan_info() if (has_band or not f32) else (1, 0)
            out.update({tag + "_ms": round(med, 4), tag + "_min_ms": round(lo, 4), tag + "_max_ms": round(hi, 4), tag + "_plan_kind": kind,
                        tag + "_plan_bytes": nbytes, tag + "_plan_build_ms": round(build * 1e3, 2)})
            return med
        finally:
            for k in opts:
                sprs_amd.set_option(k, 0)

    tile = variant("f32_tile", {"spmv_band": 2} if has_band else {}, True)
    # streamed bytes the algorithm needs: values + indices + indptr + x once + y once
    b32 = nnz * (4 + indices.element_size()) + (n + 1) * indptr.element_size() + 2 * n * 4
    out.update(f32_tile_algorithmic_GBps=round(b32 / tile / 1e6, 1))
    if has_band:
        variant("f32_auto", {}, True)
        y_auto = y32.clone()
        variant("f32_band16k", {"spmv_band": 1, "spmv_f32_band_tile": 16384}, True)
        variant("f32_band32k", {"spmv_band": 1, "spmv_f32_band_tile": 32768}, True)
    variant("f64_tile", {"spmv_xcs": 2}, False)
    assert out["f64_tile_plan_kind"] == 1
    variant("f64_default", {}, False)
    # the f32 result (the last f32 variant's) against the f64 one of the same inputs (u = 2^-24 per rounding)
    out.update(max_abs_diff_f32_vs_f64=(y32.double() - y64).abs().max().item())
    if has_band:
        out.update(max_abs_diff_f32_auto_vs_f64=(y_auto.double() - y64).abs().max().item())
    return out


def matrix(which, dev):
    import torch
    from sprs_amd import gen
    if which == "lap":
        g = 4096
        return ("5-pt Laplacian %d^2" % g, g * g) + tuple(gen.grid_laplacian(g, g, device=dev, idx_dtype=torch.int32, ptr_dtype=torch.int32))
    n = {"rmat1m": 1_000_000, "rmat10m": 10_000_000}[which]
    return ("R-MAT %dM x 16" % (n // 1_000_000), n) + tuple(gen.rmat_csr(n, 16, device=dev, idx_dtype=torch.int32, ptr_dtype=torch.int32))


def run_once(reps, inner, matrices):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("spmv_f32_bench.py: no GPU — nothing is measured without one")
    dev = torch.device("cuda", 0)
    lines = []
    for which in matrices:
        name, n, ip, ix, dt = matrix(which, dev)
        lines.append(measure(name, n, ip, ix, dt, reps, inner))
        del ip, ix, dt
        torch.cuda.empty_cache()
    out_dir = os.environ.get("SPMV_F32_BENCH_OUT", os.path.join(ROOT, "profiles"))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "spmv_f32_bench.jsonl"), "w") as f:
        for line in lines:
            s = json.dumps(line)
            print(s, flush=True)
            f.write(s + "\n")


def run_ab(reps, inner, matrices, parent_tree, runs):
    out_dir = os.environ.get("SPMV_F32_BENCH_OUT", os.path.join(ROOT, "profiles"))
    os.makedirs(out_dir, exist_ok=True)
    trees = (("parent", parent_tree), ("new", ROOT))
    seen = {}                                                        # (matrix, variant tree, key) -> values over the runs
    with open(os.path.join(out_dir, "spmv_f32_band_ab.txt"), "w") as f:
        def emit(s):
            print(s, flush=True)
            f.write(s + "\n")
            f.flush()
        emit("# f32 banded SpMV plan: A/B against the parent commit, one process per run, the two libraries alternating in one session")
        emit("# (parent = library and package of the parent commit; new = this tree).  command per run: spmv_f32_bench.py %d %d --matrices %s"
             % (reps, inner, ",".join(matrices)))
        for run in range(runs):
            for tag, tree in trees:
                env = dict(os.environ, SPMV_F32_BENCH_OUT=os.path.join(out_dir, "ab_tmp_" + tag))
                env.pop("SPRS_HIP_LIBRARY", None)
                r = subprocess.run([sys.executable, os.path.join(tree, "scripts", "spmv_f32_bench.py"), str(reps), str(inner), "--matrices",
                                    ",".join(matrices)], cwd=tree, env=env, capture_output=True, text=True, timeout=900)
                if r.returncode != 0:                                # (a fault ends the session here: nothing more is started)
                    emit("# run %d of %s FAILED with status %d: %s" % (run, tag, r.returncode, r.stderr[-400:].replace("\n", " | ")))
                    return 1
                for ln in r.stdout.splitlines():
                    if not ln.startswith("{"):
                        continue
                    rec = json.loads(ln)
                    emit(json.dumps(dict(run=run, variant=tag, **rec)))
                    for k, v in rec.items():
                        if k.endswith("_ms") and not k.endswith(("_min_ms", "_max_ms")):
                            seen.setdefault((rec["matrix"], tag, k), []).append(v)
        emit("# ---- over the runs: median [min .. max] of the per-run medians, ms")
        for (mat, tag, k), v in sorted(seen.items()):
            emit("# %-22s %-6s %-24s %.4f [%.4f .. %.4f]  (%d runs)" % (mat, tag, k, statistics.median(v), min(v), max(v), len(v)))
    return 0


def main():
    args = sys.argv[1:]
    matrices, ab = list(MATRICES), None
    if "--matrices" in args:
        i = args.index("--matrices")
        matrices = args[i + 1].split(",")
        assert all(m in MATRICES for m in matrices), matrices
        del args[i:i + 2]
    if "--ab" in args:
        i = args.index("--ab")
        ab = (os.path.abspath(args[i + 1]), int(args[i + 2]))
        del args[i:i + 3]
    reps = int(args[0]) if len(args) > 0 else 15
    inner = int(args[1]) if len(args) > 1 else 20
    if ab:
        raise SystemExit(run_ab(reps, inner, matrices, *ab))
    sys.path.insert(0, ROOT)
    run_once(reps, inner, matrices)


if __name__ == "__main__":
    main()
