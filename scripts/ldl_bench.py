#!/usr/bin/env python3
"""LDL^T timing (sprs_amd/csrc/ldl.hpp) on matrices that stay on the device:
  * 5-point Laplacians of g x g grids (symmetric, diagonal 4.5) under reverse Cuthill-McKee: a banded L with ~g entries per row,
    an elimination tree that is nearly a path — the numeric pass pipelines rows through the hand-off, and
  * a block-diagonal forest: `blocks` dense symmetric blocks of `bsize`, no reduction — thousands of roots, independent rows.
Each line reports n, nnz(A), nnz(L), the symbolic pass's counters (launches of the elimination-tree pass, all launches, host
read-backs) and the times of the ordering, symbolic, factor, update and solve calls.
Timed with the host clock around blocking calls, median of `reps` runs after one warm-up.  One JSON line per case.
usage: ldl_bench.py [--grids 64,128,256] [--blocks 4096] [--bsize 8] [--reps 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sprs_amd                                                     # noqa: E402
from sprs_amd import FillInReduction, Ldl, LdlSymbolic, SymmetryCheck  # noqa: E402
from sprs_amd._ffi import check, lib                                # noqa: E402
from sprs_amd.device import DeviceCsMat, DeviceVec                  # noqa: E402


def timed(call, reps):
    call()
    out = []
    for _ in range(reps):
        check(lib.sprs_hip_synchronize(None))
        t0 = time.perf_counter()
        res = call()
        check(lib.sprs_hip_synchronize(None))
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), res


def grid_laplacian(g):
    idx = np.arange(g * g, dtype=np.int64).reshape(g, g)
    rows = [idx.ravel()]
    cols = [idx.ravel()]
    vals = [np.full(g * g, 4.5)]
    for a, b in ((idx[:, :-1], idx[:, 1:]), (idx[:-1, :], idx[1:, :])):
        for r, c in ((a, b), (b, a)):
            rows.append(r.ravel())
            cols.append(c.ravel())
            vals.append(np.full(r.size, -1.0))
    return csr(g * g, np.concatenate(rows), np.concatenate(cols), np.concatenate(vals))


def forest(blocks, bsize, seed=1):
    rng = np.random.RandomState(seed)
    blk = rng.standard_normal((blocks, bsize, bsize))
    blk = blk + blk.transpose(0, 2, 1)
    blk[:, np.arange(bsize), np.arange(bsize)] = 4.0 * bsize + rng.rand(blocks, bsize)
    base = (np.arange(blocks) * bsize)[:, None, None]
    rows = np.broadcast_to(base + np.arange(bsize)[None, :, None], blk.shape)
    cols = np.broadcast_to(base + np.arange(bsize)[None, None, :], blk.shape)
    return csr(blocks * bsize, rows.ravel(), cols.ravel(), blk.ravel())


def csr(n, rows, cols, vals):
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    indptr = np.zeros(n + 1, dtype=np.uint32)
    indptr[1:] = np.cumsum(np.bincount(rows, minlength=n))
    return DeviceCsMat.from_host((n, n), indptr, cols.astype(np.uint32), vals.astype(np.float64))


def case(name, a, builder, reps):
    n = a.rows()
    row = {"case": name, "n": n, "nnz": a.nnz(), "lds_cap": sprs_amd.get_option("ldl_lds_cap")}
    ms, perm = timed(lambda: builder.perm(a), reps)
    row["perm_ms"] = round(ms, 2)
    ms, sym = timed(lambda: LdlSymbolic.new_perm(a, perm, SymmetryCheck.CheckSymmetry), reps)
    row["symbolic_ms"], row["nnz_l"] = round(ms, 2), sym.nnz()
    row.update(sym.stats)
    ms, num = timed(lambda: sym.factor(a), reps)
    row["factor_ms"] = round(ms, 2)
    ms, _ = timed(lambda: num.update(a), reps)
    row["update_ms"] = round(ms, 2)
    b = DeviceVec.from_host(np.random.RandomState(2).standard_normal(n))
    x = DeviceVec(n)
    ms_first = time.perf_counter()
    num.solve(b, out=x)                                              # builds the two level plans
    check(lib.sprs_hip_synchronize(None))
    row["first_solve_ms"] = round((time.perf_counter() - ms_first) * 1e3, 2)
    ms, _ = timed(lambda: num.solve(b, out=x), reps)
    row["solve_ms"] = round(ms, 2)
    r = (a * x).to_host() - b.to_host()
    row["residual_max"] = float(np.abs(r).max())
    print(json.dumps(row), flush=True)
    sprs_amd.pool_trim()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", default="64,128,256")
    ap.add_argument("--blocks", type=int, default=4096)
    ap.add_argument("--bsize", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    for g in [int(t) for t in args.grids.split(",") if t]:
        case("laplacian %d^2 rcm" % g, grid_laplacian(g), Ldl().fill_in_reduction(FillInReduction.ReverseCuthillMcKee), args.reps)
    if args.blocks:
        case("forest %d x %d" % (args.blocks, args.bsize), forest(args.blocks, args.bsize),
             Ldl().fill_in_reduction(FillInReduction.NoReduction), args.reps)


if __name__ == "__main__":
    main()
