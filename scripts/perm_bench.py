#!/usr/bin/env python3
"""Permutation timing (sprs_hip_csmat_transform_papt / sprs_hip_csmat_transform_paq, sprs_amd/csrc/perm.hpp) on the project's two
bench matrices — R-MAT (default n = 10M, ~32 per row) and the 5-point Laplacian of a 4096^2 grid — under a seeded random
permutation: transform_mat_papt (both sides: every slice is relabelled and sorted) and rows-only permute_rows (the copy path).
Each is timed beside the two routes a user had before:
  (a) triplets   relabel the (row, col) pairs on the device, then sprs_hip_triplets_to_cs (a global radix sort of 64-bit keys)
  (b) host       download A, permute with numpy, upload (one run; skipped above --host-max-nnz entries: the numpy sort alone
                 takes minutes there)
Algorithmic bytes of one permutation: the indptr read and written, both maps read, 12 B read and 12 B written per entry
(4-byte indices, 8-byte values).  Warm, timed with events on the stream, median of `reps` runs.  One JSON line per case.
usage: perm_bench.py [n] [nnz_per_row] [reps] [--host-max-nnz N] [--grid G]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sprs_amd                                       # noqa: E402
from sprs_amd import _ffi, gen, permutation           # noqa: E402
from sprs_amd.device import DeviceCsMat               # noqa: E402
from sprs_amd.permutation import DevicePerm           # noqa: E402

S_I, S_P = 4, 8


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


def class_shares(indptr, cap):
    """share of the entries in rows of <= 16, <= 32, <= 64, <= 1024 (one wave sorts the row), <= cap (a workgroup) and more entries"""
    lens = indptr[1:] - indptr[:-1]
    total = max(1, int(lens.sum()))
    edges = [0, 16, 32, 64, 1024, cap, 1 << 62]
    return {("<=%d" % hi if hi < 1 << 62 else ">%d" % cap): round(int(lens[(lens > lo) & (lens <= hi)].sum()) / total, 4)
            for lo, hi in zip(edges[:-1], edges[1:])}


def triplet_route(n, indptr, indices, data, inv, relabel_cols):
    """route (a): relabelled triplets -> sprs_hip_triplets_to_cs (CSR, 4-byte indices, 8-byte indptr)"""
    row_of = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=indptr.device), indptr[1:] - indptr[:-1])
    rows = inv[row_of]
    cols = inv[indices.to(torch.int64)] if relabel_cols else indices.to(torch.int64)
    h = C.c_void_p()
    _ffi.check(_ffi.lib.sprs_hip_triplets_to_cs(n, n, rows.numel(), C.c_void_p(rows.data_ptr()), C.c_void_p(cols.data_ptr()), 8,
                                                C.c_void_p(data.data_ptr()), _ffi.CSR, S_I, S_P, C.byref(h)))
    return DeviceCsMat(h.value)


def host_route(a, perm, both):
    """route (b): download, numpy, upload"""
    t0 = time.perf_counter()
    shape, ip, ix, dt = a.to_host()
    ip = ip.astype(np.int64)
    n = shape[0]
    lens = (ip[1:] - ip[:-1])[perm]
    nip = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=nip[1:])
    src = np.repeat(ip[perm] - nip[:-1], lens) + np.arange(nip[-1])
    nix, ndt = ix[src], dt[src]
    if both:
        inv = np.empty(n, dtype=np.int64)
        inv[perm] = np.arange(n)
        nix = inv[nix]
        order = np.argsort(np.repeat(np.arange(n), lens) * n + nix, kind="stable")
        nix, ndt = nix[order], ndt[order]
    res = DeviceCsMat.from_host(shape, nip.astype(np.uint64), nix.astype(np.uint32), ndt, validate=False)
    return res, (time.perf_counter() - t0) * 1e3


def same_structure(x, y):
    r, c, nnz, pb, ib, st = x._info()
    if (r, c, nnz) != y._info()[:3]:
        return False
    a, b = np.empty(r + 1, dtype=np.uint64), np.empty(r + 1, dtype=np.uint64)
    _ffi.check(_ffi.lib.sprs_hip_csmat_download(x._h, C.c_void_p(a.ctypes.data), None, None))
    _ffi.check(_ffi.lib.sprs_hip_csmat_download(y._h, C.c_void_p(b.ctypes.data), None, None))
    return bool(np.array_equal(a, b))


def case(name, n, indptr, indices, data, reps, host_max, cap):
    dev = indptr.device
    indices = indices.to(torch.int32)
    a = DeviceCsMat.wrap_torch((n, n), indptr, indices, data)
    nnz = indices.numel()
    g = torch.Generator(device="cpu")
    g.manual_seed(1234)
    hperm = torch.randperm(n, generator=g)
    tperm = hperm.to(dev).to(torch.int32)
    p = DevicePerm.from_device(tperm)
    inv = torch.empty(n, dtype=torch.int64, device=dev)
    inv[tperm.to(torch.int64)] = torch.arange(n, dtype=torch.int64, device=dev)
    nbytes = 2 * (n + 1) * S_P + nnz * 2 * (8 + S_I)
    shares = class_shares(indptr, cap)
    for op, both in (("transform_mat_papt", True), ("permute_rows", False)):
        call = (lambda: permutation.transform_mat_papt(a, p)) if both else (lambda: permutation.permute_rows(a, p))
        res = call()
        tri = triplet_route(n, indptr, indices, data, inv, both)
        assert same_structure(res, tri), "the dedicated path and the triplet route disagree"
        del tri
        ms = median_ms(call, reps)
        ms_tri = median_ms(lambda: triplet_route(n, indptr, indices, data, inv, both), reps)
        row = {"case": name, "op": op, "n": n, "nnz": nnz, "ms": round(ms, 3), "triplet_route_ms": round(ms_tri, 3),
               "speedup_over_triplets": round(ms_tri / ms, 2),
               "algorithmic_bytes": nbytes + (2 if both else 1) * n * S_I,
               "nnz_share_by_row_length": shares}
        row["algorithmic_GBs"] = round(row["algorithmic_bytes"] / ms / 1e6, 1)
        row["frac_of_8TBs"] = round(row["algorithmic_bytes"] / (ms * 1e-3) / 8e12, 4)
        if nnz <= host_max:
            hres, hms = host_route(a, hperm.numpy(), both)
            assert same_structure(res, hres)
            row["host_route_ms"] = round(hms, 1)
            del hres
        else:
            row["host_route_ms"] = None
        print(json.dumps(row), flush=True)
        del res
    torch.cuda.empty_cache()
    sprs_amd.pool_trim()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", nargs="?", type=int, default=10_000_000)
    ap.add_argument("nnz_per_row", nargs="?", type=float, default=32)
    ap.add_argument("reps", nargs="?", type=int, default=5)
    ap.add_argument("--host-max-nnz", type=int, default=120_000_000)
    ap.add_argument("--grid", type=int, default=4096)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cap = int(sprs_amd.get_option("perm_cap"))
    ip, ix, dt = gen.rmat_csr(args.n, args.nnz_per_row, seed=1, value_seed=2, device=dev)
    case("rmat n=%d" % args.n, args.n, ip, ix, dt, args.reps, args.host_max_nnz, cap)
    del ip, ix, dt
    torch.cuda.empty_cache()
    if args.grid:
        g = args.grid
        ip, ix, dt = gen.grid_laplacian(g, g, device=dev)
        case("laplacian %d^2" % g, g * g, ip, ix, dt, args.reps, args.host_max_nnz, cap)


if __name__ == "__main__":
    main()
