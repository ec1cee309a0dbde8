#!/usr/bin/env python3
"""The device reductions and extraction (csvec_reduce.hpp, extract.hpp) beside the host round trip each replaces: to_host plus
the numpy restatement (np.cumsum adds left to right, so its last element is the reference's chain).
  * the ordered chain (squared_l2_norm) at nnz = 1e3, 1e5, 1e7, in ns per stored entry;
  * dot of two sparse vectors of 1e5 entries with 10 % overlap;
  * diag and to_inner_onehot on the 1024 x 1024 grid Laplacian, an R-MAT matrix of 2^20 rows, and one matrix with a 1e6-entry hub
    slice among 1e6 short ones (whether the whole-wave rule for hub slices holds).
Warm, REPEATS timed calls each, median and [min, max]; every device result is checked against the restatement first.  One JSON
line per case.
usage: reduce_bench.py [scale]     (scale < 1 shrinks every size, for a rehearsal)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sprs_amd import gen                                           # noqa: E402
from sprs_amd.device import DeviceCsMat, DeviceCsVec               # noqa: E402

REPEATS = 9


def timed(f):
    f()                                                            # warm: code objects, the pool's blocks
    ts = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        f()                                                        # every call here returns a host value: complete at return
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), min(ts), max(ts)


def report(case, nnz, dev, host, **extra):
    print(json.dumps(dict({"case": case, "nnz": int(nnz), "device_ms": round(dev[0] * 1e3, 4),
                           "device_ms_min_max": [round(dev[1] * 1e3, 4), round(dev[2] * 1e3, 4)],
                           "device_ns_per_entry": round(dev[0] * 1e9 / max(nnz, 1), 3),
                           "host_round_trip_ms": round(host[0] * 1e3, 4), "repeats": REPEATS}, **extra)), flush=True)


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def chain_case(n):
    rng = np.random.default_rng(n)
    idx = np.arange(n, dtype=np.uint64) * 3
    data = rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 8, n)
    v = DeviceCsVec.from_host(3 * n, idx, data, validate=False)

    def host():
        _, _, d = v.to_host()
        return float(np.cumsum(d * d)[-1])
    assert bits(v.squared_l2_norm()) == bits(host()), "chain differs from the restatement at n = %d" % n
    report("squared_l2_norm (the ordered chain)", n, timed(v.squared_l2_norm), timed(host))


def dot_case(n):
    rng = np.random.default_rng(7)
    dim = 20 * n
    pool = rng.choice(dim, 2 * n - n // 10, replace=False)
    ai, bi = np.sort(pool[:n]), np.sort(np.concatenate([pool[:n // 10], pool[n:]]))
    a = DeviceCsVec.from_host(dim, ai.astype(np.uint64), rng.standard_normal(n), validate=False)
    b = DeviceCsVec.from_host(dim, bi.astype(np.uint64), rng.standard_normal(n), validate=False)

    def host():
        _, i1, d1 = a.to_host()
        _, i2, d2 = b.to_host()
        _, p1, p2 = np.intersect1d(i1, i2, assume_unique=True, return_indices=True)
        return float(np.cumsum(d1[p1] * d2[p2])[-1])
    assert bits(a.dot(b)) == bits(host())
    report("dot, two sparse vectors, 10 % overlap", n, timed(lambda: a.dot(b)), timed(host))


def host_diag(shape, ip, ix, dt):
    row_of = np.repeat(np.arange(ip.size - 1, dtype=np.int64), np.diff(ip.astype(np.int64)))
    hit = ix.astype(np.int64) == row_of
    return row_of[hit], dt[hit]


def host_onehot(ip, ix, dt):
    """per slice the last maximal non-NaN entry: a stable sort by (slice, value) puts it last in its slice"""
    ip = ip.astype(np.int64)
    row_of = np.repeat(np.arange(ip.size - 1, dtype=np.int64), np.diff(ip))
    ok = ~np.isnan(dt)
    r, x, k = row_of[ok], dt[ok] + 0.0, ix[ok]                     # (+ 0.0 leaves -0.0 alone; lexsort holds -0.0 == 0.0)
    order = np.lexsort((x, r))
    r, k = r[order], k[order]
    last = np.ones(r.size, dtype=bool)
    last[:-1] = r[1:] != r[:-1]
    counts = np.zeros(ip.size, dtype=np.int64)
    np.add.at(counts, r[last] + 1, 1)
    return np.cumsum(counts), k[last]


def matrix_case(name, shape, ip, ix, dt):
    m = DeviceCsMat.from_host(shape, ip, ix, dt, validate=False)

    def host_d():
        _, a, b, c = m.to_host()
        return host_diag(shape, a, b, c)

    def host_o():
        _, a, b, c = m.to_host()
        return host_onehot(a, b, c)
    _, di, dd = m.diag().to_host()
    hi, hd = host_d()
    assert np.array_equal(di.astype(np.int64), hi) and np.array_equal(bits(dd), bits(hd)), "diag differs: " + name
    _, oip, oix, _ = m.to_inner_onehot().to_host()
    hip, hix = host_o()
    assert np.array_equal(oip.astype(np.int64), hip) and np.array_equal(oix.astype(np.int64), hix.astype(np.int64)), "onehot differs: " + name
    longest = int(np.diff(ip.astype(np.int64)).max())
    report("diag, " + name, ix.size, timed(m.diag), timed(host_d), outer=int(ip.size - 1), longest_slice=longest)
    report("to_inner_onehot, " + name, ix.size, timed(m.to_inner_onehot), timed(host_o), outer=int(ip.size - 1), longest_slice=longest)


def hub_matrix(n_short, hub_len):
    """n_short slices of 3 entries (the diagonal among them) and, in the middle, one slice of hub_len entries"""
    cols = max(hub_len, n_short + 1)
    rng = np.random.default_rng(3)
    lens = np.full(n_short + 1, 3, dtype=np.int64)
    hub = n_short // 2
    lens[hub] = hub_len
    ip = np.zeros(n_short + 2, dtype=np.uint64)
    ip[1:] = np.cumsum(lens)
    ix = np.empty(int(ip[-1]), dtype=np.uint64)
    rows = np.arange(n_short + 1)
    short = rows != hub
    base = np.minimum(rows[short], cols - 3)
    starts = ip[:-1][short].astype(np.int64)
    for k in range(3):
        ix[starts + k] = base + k
    ix[int(ip[hub]):int(ip[hub + 1])] = np.arange(hub_len)
    return (n_short + 1, cols), ip, ix, rng.standard_normal(ix.size)


def main():
    scale = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
    for n in (1000, 100000, 10000000):
        chain_case(max(int(n * scale), 70))
    dot_case(max(int(100000 * scale), 100))
    g = max(int(1024 * scale ** 0.5), 8)
    ip, ix, dt = gen.grid_laplacian(g, g)
    matrix_case("%d x %d grid Laplacian" % (g, g), (g * g, g * g), ip.numpy().astype(np.uint64), ix.numpy().astype(np.uint64), dt.numpy())
    rows = max(int((1 << 20) * scale), 64)
    ip, ix, dt = gen.rmat_csr(rows, 8)
    matrix_case("R-MAT %d rows, 8 per row" % rows, (rows, rows), ip.numpy().astype(np.uint64), ix.numpy().astype(np.uint64), dt.numpy())
    n = max(int(1000000 * scale), 200)
    matrix_case("hub slice of %d entries among %d short ones" % (n, n), *hub_matrix(n, n))


if __name__ == "__main__":
    main()
