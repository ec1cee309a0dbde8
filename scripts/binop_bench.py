#!/usr/bin/env python3
"""Sparse + sparse timing (sprs_hip_csmat_add_csmat_f64 and friends, sprs_amd/csrc/binop.hpp) on three cases:
  rmat      A + B, two R-MAT n x n matrices of different seeds (default n = 10M, ~32 per row: the bench matrix)
  uniform   A + B, the same nnz with every row equally long
  heat      I - 0.1 * L on the 5-point Laplacian of a 4096^2 grid (scale, then subtract)
Algorithmic bytes of one binop = both operands read TWICE (the counting and the emitting pass) + the result written once:
  2 * (nnzA + nnzB) * (8 + S_I) + 4 * (outer + 1) * S_P + nnzC * (8 + S_I) + (outer + 1) * S_P.
The yardstick is measured in the same run: a device-to-device copy that MOVES that many bytes (a buffer of half of them,
read once and written once).  One JSON line per case, then the R-MAT / uniform time ratio.
usage: binop_bench.py [n] [nnz_per_row] [reps]"""
import ctypes as C
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sprs_amd import _ffi, gen                       # noqa: E402
from sprs_amd.device import DeviceCsMat              # noqa: E402

S_I = S_P = 8


def timed(call, reps):
    """the calls block until their result is complete on the stream: wall time is device time + launch / read-back latency"""
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def copy_seconds(nbytes, reps, dev):
    """a device-to-device copy that moves nbytes in all (reads nbytes / 2, writes nbytes / 2)"""
    half = max(8, nbytes // 2 // 8 * 8)
    src = torch.empty(half // 8, dtype=torch.float64, device=dev).fill_(1.0)
    dst = torch.empty_like(src)
    call = lambda: (_ffi.check(_ffi.lib.sprs_hip_memcpy_d2d(C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), half, None)),
                    _ffi.check(_ffi.lib.sprs_hip_synchronize(None)))
    return timed(call, reps)


def binop_bytes(outer, nnz_a, nnz_b, nnz_c):
    return 2 * (nnz_a + nnz_b) * (8 + S_I) + 4 * (outer + 1) * S_P + nnz_c * (8 + S_I) + (outer + 1) * S_P


def uniform_rows(n, k, seed, dev):
    """n x n, exactly k entries in every row: entry j of a row sits in the j-th of k equal column ranges, at a hashed offset"""
    width = n // k
    e = torch.arange(n * k, dtype=torch.int64, device=dev)
    j = e % k
    col = j * width + gen._lsr(gen.splitmix64(e, seed), 1) % width
    indptr = torch.arange(n + 1, dtype=torch.int64, device=dev) * k
    return indptr, col, gen.uniform_05_15(e, seed + 1)


def report(name, outer, a, b, seconds, c, reps, dev, extra=None):
    nbytes = binop_bytes(outer, a.nnz(), b.nnz(), c.nnz())
    cp = copy_seconds(nbytes, reps, dev)
    row = {"case": name, "outer": outer, "nnz_a": a.nnz(), "nnz_b": b.nnz(), "nnz_c": c.nnz(), "ms": round(seconds * 1e3, 3),
           "algorithmic_bytes": nbytes, "algorithmic_GBs": round(nbytes / seconds / 1e9, 1), "frac_of_8TBs": round(nbytes / seconds / 8e12, 4),
           "copy_same_bytes_ms": round(cp * 1e3, 3), "copy_GBs": round(nbytes / cp / 1e9, 1), "time_over_copy": round(seconds / cp, 2)}
    row.update(extra or {})
    print(json.dumps(row), flush=True)
    return row


def add_case(name, ma, mb, n, reps, dev):
    a = DeviceCsMat.wrap_torch((n, n), *ma)
    b = DeviceCsMat.wrap_torch((n, n), *mb)
    c = a + b
    # every value is positive (0.5 .. 1.5): nothing cancels, so nnz(C) = nnz(A) + nnz(B) - shared indices, and the values add up
    h = c.to_host() if c.nnz() <= 1 << 22 else None
    if h is not None:
        assert abs(h[3].sum() - float(ma[2].sum() + mb[2].sum())) <= 1e-9 * h[3].sum()
    seconds = timed(lambda: a + b, reps)
    return report(name, n, a, b, seconds, c, reps, dev)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    k = float(sys.argv[2]) if len(sys.argv) > 2 else 32
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    dev = torch.device("cuda", 0)

    ma = gen.rmat_csr(n, k, seed=1, value_seed=2, device=dev)
    mb = gen.rmat_csr(n, k, seed=21, value_seed=22, device=dev)
    rmat = add_case("rmat A + B", ma, mb, n, reps, dev)
    ku = max(1, int(round((ma[1].numel() + mb[1].numel()) / 2 / n)))
    del ma, mb
    torch.cuda.empty_cache()

    ua, ub = uniform_rows(n, ku, 31, dev), uniform_rows(n, ku, 41, dev)
    uni = add_case("uniform rows A + B", ua, ub, n, reps, dev)
    del ua, ub
    torch.cuda.empty_cache()
    per_slot = lambda r: r["ms"] / (r["nnz_a"] + r["nnz_b"])
    print(json.dumps({"rmat_over_uniform_time": round(rmat["ms"] / uni["ms"], 3),
                      "rmat_over_uniform_time_per_slot": round(per_slot(rmat) / per_slot(uni), 3)}), flush=True)

    g = 4096
    lap = DeviceCsMat.wrap_torch((g * g, g * g), *gen.grid_laplacian(g, g, device=dev))
    eye = DeviceCsMat.wrap_torch((g * g, g * g), torch.arange(g * g + 1, dtype=torch.int64, device=dev),
                                 torch.arange(g * g, dtype=torch.int64, device=dev), torch.ones(g * g, dtype=torch.float64, device=dev))
    scaled = lap * 0.1
    step = eye - scaled
    t_scale = timed(lambda: lap * 0.1, reps)
    t_sub = timed(lambda: eye - scaled, reps)
    scale_bytes = lap.nnz() * (2 * 8 + 2 * S_I) + 2 * (g * g + 1) * S_P
    report("heat I - 0.1 L (the subtraction)", g * g, eye, scaled, t_sub, step, reps, dev,
           {"scale_ms": round(t_scale * 1e3, 3), "scale_bytes": scale_bytes, "scale_GBs": round(scale_bytes / t_scale / 1e9, 1),
            "scale_copy_same_bytes_ms": round(copy_seconds(scale_bytes, reps, dev) * 1e3, 3),
            "both_ms": round((t_scale + t_sub) * 1e3, 3)})


if __name__ == "__main__":
    main()
