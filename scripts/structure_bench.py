#!/usr/bin/env python3
"""Structure-check and new_from_unsorted timing (sprs_hip_csmat_check_structure / sprs_hip_csmat_from_unsorted,
sprs_amd/csrc/structure.hpp) on the project's R-MAT bench matrix (default n = 10M, ~32 per row; 4-byte indices, 8-byte indptr),
once with every row shuffled and once with no row shuffled:
  check          the indptr pass and the nnz-tiled row pass (on the shuffled matrix it ends in "Indices are not sorted": same work)
  from_unsorted  shuffled: flag pass, copy, the masked sorts by length class, the check of the result
                 sorted:   flag pass and a copy
Beside them permute_cols (transform_mat_paq with a NULL row side) under a seeded random column permutation on the same matrix:
the permutation code doing the same gather-and-sort work plus a lookup of every index.
Algorithmic bytes of the check: the indptr and the indices read once.  Of from_unsorted: the indptr read and written, 12 B read
and 12 B written per entry.  Warm, timed with events on the stream, median of `reps` runs.  One JSON line per case.
usage: structure_bench.py [n] [nnz_per_row] [reps]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sprs_amd                                       # noqa: E402
from sprs_amd import SprsHipError, _ffi, gen, permutation   # noqa: E402
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


def shuffle_rows(n, indptr, indices, data, seed):
    """every row's entries in a seeded random order (values travel with their indices)"""
    g = torch.Generator(device=indptr.device)
    g.manual_seed(seed)
    row_of = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=indptr.device), indptr[1:] - indptr[:-1])
    key = (row_of << 31) | torch.randint(0, 1 << 31, (indices.numel(),), generator=g, device=indptr.device, dtype=torch.int64)
    order = torch.argsort(key)
    return indices[order].contiguous(), data[order].contiguous()


def emit(name, op, n, nnz, ms, nbytes, **more):
    row = {"case": name, "op": op, "n": n, "nnz": nnz, "ms": round(ms, 3), "algorithmic_bytes": nbytes,
           "algorithmic_GBs": round(nbytes / ms / 1e6, 1), "frac_of_8TBs": round(nbytes / (ms * 1e-3) / 8e12, 4)}
    row.update(more)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", nargs="?", type=int, default=10_000_000)
    ap.add_argument("nnz_per_row", nargs="?", type=float, default=32)
    ap.add_argument("reps", nargs="?", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = args.n
    ip, ix, dt = gen.rmat_csr(n, args.nnz_per_row, seed=1, value_seed=2, device=dev)
    ix = ix.to(torch.int32)
    nnz = ix.numel()
    name = "rmat n=%d" % n
    check_bytes = (n + 1) * S_P + nnz * S_I
    sort_bytes = 2 * (n + 1) * S_P + nnz * 2 * (8 + S_I)
    a = DeviceCsMat.wrap_torch((n, n), ip, ix, dt)
    a.check_structure()

    def failing_check(m):
        try:
            m.check_structure()
        except SprsHipError:
            return
        raise AssertionError("a shuffled matrix passed the check")

    emit(name, "check sorted", n, nnz, median_ms(a.check_structure, args.reps), check_bytes)
    emit(name, "from_unsorted sorted", n, nnz, median_ms(a.sort_indices, args.reps), sort_bytes)
    g = torch.Generator(device="cpu")
    g.manual_seed(1234)
    q = DevicePerm.from_device(torch.randperm(n, generator=g).to(dev).to(torch.int32))
    emit(name, "permute_cols random", n, nnz, median_ms(lambda: permutation.permute_cols(a, q), args.reps), sort_bytes + n * S_I)
    del q
    six, sdt = shuffle_rows(n, ip, ix, dt, 99)
    s = DeviceCsMat.wrap_torch((n, n), ip, six, sdt)
    res = s.sort_indices()
    rix = np.empty(nnz, dtype=np.uint32)
    _ffi.check(_ffi.lib.sprs_hip_csmat_download(res._h, None, C.c_void_p(rix.ctypes.data), None))
    assert np.array_equal(rix, ix.cpu().numpy().view(np.uint32)), "from_unsorted of the shuffled matrix is not the sorted matrix"
    del res, rix
    emit(name, "check shuffled", n, nnz, median_ms(lambda: failing_check(s), args.reps), check_bytes)
    emit(name, "from_unsorted shuffled", n, nnz, median_ms(s.sort_indices, args.reps), sort_bytes)
    torch.cuda.empty_cache()
    sprs_amd.pool_trim()


if __name__ == "__main__":
    main()
