"""Sparse-vector products on the device: CSR x v, CSC x v, v x CSR, v x CSC (sprs_hip_csmat_mul_csvec_f64 /
sprs_hip_csvec_mul_csmat_f64) on R-MAT matrices, for v of densities 1e-6 .. 1.

One JSON line per (matrix, density, operator): median ms of --reps calls (each call returns with the result complete), the
model bytes

    (m+1)*w_ptr + nnz*w_idx + 16*matches + nnz(v)*(w_idx+8) + n/8 + nnz(out)*(w_idx+8)

(one pass over the indptr and indices of the operand the kernel runs on, M's value and v's value of every matched entry, v
itself, its presence bitmap, the result), the fraction of 8 TB/s they represent, and the longest serial chain: the most matched
entries of one outer slice, whose ordered sum is a chain of dependent adds.  Also: the longest row / column of the matrix and the
time of the first (un-prepared) SpMV of a fresh handle on the same arrays, the yardstick of density 1.

    python scripts/csvec_bench.py [--matrices rmat10m,rmat10m_u32,rmat1m] [--densities 1e-6,1e-4,1e-2,0.1,1] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import sprs_amd  # noqa: E402
from sprs_amd import gen, prod  # noqa: E402
from sprs_amd.device import DeviceCsMat, DeviceCsVec, DeviceVec  # noqa: E402

MATRICES = {
    "rmat10m": (10_000_000, 32, torch.int64),
    "rmat10m_u32": (10_000_000, 32, torch.int32),
    "rmat1m": (1_000_000, 16, torch.int64),
}


def chain_stats(ip, ix, present):
    """(matched entries, longest chain) of the masked dot over the outer slices of (ip, ix)"""
    hit = present[ix.long()].to(torch.int64)
    c = torch.zeros(hit.numel() + 1, dtype=torch.int64, device=hit.device)
    torch.cumsum(hit, 0, out=c[1:])
    ipl = ip.long()
    per = c[ipl[1:]] - c[ipl[:-1]]
    return int(c[-1]), int(per.max()) if per.numel() else 0


def timed(fn, reps):
    fn()                                  # first call: the handle's other storage form and per-handle tables
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="rmat10m,rmat10m_u32,rmat1m")
    ap.add_argument("--densities", default="1e-6,1e-4,1e-2,0.1,1")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if sprs_amd.device_count() < 1:
        sys.exit("no HIP device")
    dev = torch.device("cuda", 0)
    for name in args.matrices.split(","):
        n, k, idt = MATRICES[name]
        ip, ix, dt = gen.rmat_csr(n, k, device=dev, idx_dtype=idt, ptr_dtype=idt)
        w = ip.element_size()
        nnz = ix.numel()
        a = DeviceCsMat.wrap_torch((n, n), ip, ix, dt)
        a_csc = a.to_other_storage()
        _, cip_h, cix_h, _ = a_csc.to_host()
        cip = torch.from_numpy(cip_h.astype("int64")).to(dev)
        cix = torch.from_numpy(cix_h.astype("int64")).to(dev)
        rowlen = (ip[1:].long() - ip[:-1].long())
        collen = cip[1:] - cip[:-1]
        # the yardstick: the first SpMV of a fresh handle on the same arrays (plain tile plan)
        fresh = DeviceCsMat.wrap_torch((n, n), ip, ix, dt)
        x = DeviceVec.from_host(torch.rand(n, dtype=torch.float64).numpy())
        y = DeviceVec(n)
        torch.cuda.synchronize()
        t = time.perf_counter()
        prod.csmat_mul_vec(fresh, x, y)
        sprs_amd._ffi.lib.sprs_hip_synchronize(None)
        spmv_first_ms = (time.perf_counter() - t) * 1e3
        print(json.dumps({"matrix": name, "n": n, "nnz": nnz, "w_idx": w, "longest_row": int(rowlen.max()),
                          "longest_col": int(collen.max()), "spmv_first_unprepared_ms": round(spmv_first_ms, 4)}), flush=True)
        del fresh
        g = torch.Generator(device=dev)
        g.manual_seed(7)
        for dens in [float(d) for d in args.densities.split(",")]:
            kv = max(1, int(round(n * dens)))
            vidx = torch.arange(n, device=dev) if kv >= n else torch.sort(torch.randperm(n, device=dev, generator=g)[:kv])[0]
            vidx = vidx.to(idt)
            vval = torch.randn(vidx.numel(), dtype=torch.float64, device=dev, generator=g)
            v = DeviceCsVec.borrow(n, vidx, vval)
            present = torch.zeros(n, dtype=torch.bool, device=dev)
            present[vidx.long()] = True
            ops = (("csr_x_v", lambda: a * v, ip, ix),
                   ("csc_x_v", lambda: a_csc * v, ip, ix),          # runs on the CSR form
                   ("v_x_csr", lambda: v * a, cip, cix),            # runs on the CSC form
                   ("v_x_csc", lambda: v * a_csc, cip, cix))
            for op, fn, mip, mix in ops:
                matches, chain = chain_stats(mip, mix, present)
                ms, out = timed(fn, args.reps)
                nout = out.nnz()
                model = (n + 1) * w + nnz * w + 16 * matches + kv * (w + 8) + n / 8 + nout * (w + 8)
                print(json.dumps({"matrix": name, "density": dens, "op": op, "nnz_v": kv, "matches": matches,
                                  "longest_chain": chain, "nnz_out": nout, "ms": round(ms, 4),
                                  "model_gb": round(model / 1e9, 4), "frac_8tbs": round(model / 8e12 / (ms / 1e3), 3)}),
                      flush=True)
                del out
            del v
        del a, a_csc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
