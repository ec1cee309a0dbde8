#!/usr/bin/env python3
"""Ordering timing (sprs_hip_csmat_cuthill_mckee, sprs_amd/csrc/ordering.hpp): reverse_cuthill_mckee on a matrix that stays on
the device, and the transform_mat_papt that follows, on
  * gen.grid_laplacian, the heat example's matrix of a grid (default 4096^2: thousands of levels, up to 4096 vertices wide;
    its border rows hold a lone diagonal entry, so the pattern is NOT symmetric and is ordered along the stored direction), and
  * a symmetrised R-MAT (default n = 1M, ~8 per row), built on the device as A + A^T with the existing transpose and `&A + &B`
    (a few levels, each hundreds of thousands of vertices wide).
Each line reports components, levels of the ordering pass, launches, host read-backs and the bandwidth before and after.  Where
scipy is importable the route used before is timed too — download, scipy.sparse.csgraph.reverse_cuthill_mckee, upload of the
permutation — as a yardstick only: scipy breaks ties differently, so the permutations are not compared.
Timed with the host clock around blocking calls, median of `reps` runs after one warm-up.  One JSON line per case.
usage: ordering_bench.py [--grid G] [--rmat N] [--per-row K] [--reps R] [--no-scipy]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sprs_amd                                       # noqa: E402
from sprs_amd import gen, ordering, permutation      # noqa: E402
from sprs_amd.device import DeviceCsMat, DeviceVec    # noqa: E402
from sprs_amd.permutation import DevicePerm           # noqa: E402


def timed(call, reps):
    call()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = call()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), res


def bandwidth(a):
    shape, ip, ix, _ = a.to_host()
    rows = np.repeat(np.arange(shape[0], dtype=np.int64), np.diff(ip.astype(np.int64)))
    return int(np.abs(ix.astype(np.int64) - rows).max()) if ix.size else 0


def scipy_route(a, reps):
    try:
        import scipy.sparse as sp
        from scipy.sparse.csgraph import reverse_cuthill_mckee
    except ImportError:
        return None

    def run():
        shape, ip, ix, dt = a.to_host()
        m = sp.csr_matrix((dt, ix.astype(np.int64), ip.astype(np.int64)), shape=shape)
        perm = reverse_cuthill_mckee(m, symmetric_mode=True)
        return DevicePerm(perm.astype(np.uint32), validate=False)

    ms, _ = timed(run, max(1, reps // 2))
    return round(ms, 1)


def case(name, a, reps, with_scipy):
    n, nnz = a.rows(), a.nnz()
    row = {"case": name, "n": n, "nnz": nnz, "narrow_cap": sprs_amd.get_option("ordering_narrow_cap")}
    ms_sym, sym = timed(lambda: ordering.is_symmetric(a), reps)
    row["is_symmetric"], row["is_symmetric_ms"] = sym, round(ms_sym, 3)
    buf = DeviceVec(n)
    ms_deg, _ = timed(lambda: a.degrees(out=buf), reps)
    ms, o = timed(lambda: ordering.reverse_cuthill_mckee(a), reps)
    row["reverse_cuthill_mckee_ms"] = round(ms, 2)
    row.update(o.stats)
    ms_papt, b = timed(lambda: permutation.transform_mat_papt(a, o.perm), reps)
    row["transform_mat_papt_ms"] = round(ms_papt, 2)
    row["bandwidth_before"], row["bandwidth_after"] = bandwidth(a), bandwidth(b)
    row["degrees_ms"] = round(ms_deg, 3)
    row["scipy_download_rcm_upload_ms"] = scipy_route(a, reps) if with_scipy else None
    print(json.dumps(row), flush=True)
    del b, o
    torch.cuda.empty_cache()
    sprs_amd.pool_trim()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--rmat", type=int, default=1_000_000)
    ap.add_argument("--per-row", type=float, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-scipy", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    if args.grid:
        g = args.grid
        ip, ix, dt = gen.grid_laplacian(g, g, device=dev)
        a = DeviceCsMat.wrap_torch((g * g, g * g), ip, ix.to(torch.int32), dt)
        case("laplacian %d^2" % g, a, args.reps, not args.no_scipy)
        del a, ip, ix, dt
        torch.cuda.empty_cache()
    if args.rmat:
        n = args.rmat
        ip, ix, dt = gen.rmat_csr(n, args.per_row, seed=1, value_seed=2, device=dev)
        a = DeviceCsMat.wrap_torch((n, n), ip, ix.to(torch.int32), dt)
        s = a + a.transpose_view().to_other_storage()          # the pattern of A + A^T, on the device
        case("rmat n=%d symmetrised" % n, s, args.reps, not args.no_scipy)


if __name__ == "__main__":
    main()
