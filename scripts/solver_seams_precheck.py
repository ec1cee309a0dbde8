"""CPU pre-check of the exact-arithmetic constructions of tests/test_solver_seams_gpu.py (no device needed).

The one-step BiCGSTAB cases (A2, A3) claim that every summation order gives the same double.  That must hold for the
reference alone before a device is compared with it: for every size of the test this script runs the step
  * through the CPU oracle (serial dots),
  * through a numpy restatement of bicgstab.rs:194-229 under three summation orders — numpy's pairwise sum, a serial sum
    from the END, and the shape of the device tree (8192-element chunks, 256 strided running sums per chunk, then the
    chunks 256 at a time),
  * through the Fraction model of the test,
and requires x, err and rho to agree bit for bit.  Run:  python scripts/solver_seams_precheck.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_solver_seams_gpu as T   # noqa: E402
from oracle import oracle           # noqa: E402


def dot_pairwise(a, b):
    return float(np.sum(a * b))


def dot_from_the_end(a, b):
    return float(np.cumsum((a * b)[::-1])[-1])


def dot_tree(a, b):
    p = a * b
    pad = (-p.size) % 8192
    chunks = np.concatenate([p, np.zeros(pad)]).reshape(-1, 32, 256)
    partial = np.cumsum(chunks, axis=1)[:, -1, :]                    # thread t of a chunk: elements t, t + 256, ... in order
    partial = np.cumsum(partial[:, ::-1], axis=1)[:, -1]             # (the lanes in another order than the device's: any will do)
    pad = (-partial.size) % 256
    return float(np.cumsum(np.concatenate([partial, np.zeros(pad)]).reshape(-1, 256), axis=0)[-1].sum())


def one_step(d, b, thr, dot):
    """new() with x0 = 0 and one step(): the reference's expressions, unfused, on dense vectors"""
    r = b - d * np.zeros_like(b)
    rhat, p, x = r.copy(), r.copy(), np.zeros_like(b)
    err = np.sqrt(dot(r, r))
    rho = err * err
    v = d * p
    alpha = rho / dot(rhat, v)
    h = x + p * alpha
    s = r - v * alpha
    t = d * s
    omega = dot(t, s) / dot(t, t)
    x = h + omega * s
    r = s - t * omega
    err = np.sqrt(dot(r, r))
    rho = dot(rhat, r)
    soft = abs(rho) / (err * err) < thr
    if soft:
        rho = err * err
    return x, float(err), float(rho), int(soft)


def main():
    for name, spec in (("A2", T.STEP_PLAIN), ("A3", T.STEP_SOFT)):
        for n in T.DOT_SIZES:
            if n == 1:
                continue                                             # (the breakdown case: nothing to sum)
            d, b, sums = T.class_system(n, spec)
            ip, ix, dt = T.diag_csr(d)
            xc, err, rho, soft = T.step_model(spec, sums, 0.1)
            x_ref, info = oracle.bicgstab((n, n), ip, ix, dt, np.zeros(n), b, T.TINY_TOL, 1)
            want = (T.bits(err), T.bits(rho), soft)
            assert (T.bits(info["err"]), T.bits(info["rho"]), info["soft_restart_count"]) == want, (name, n, "oracle")
            for dot in (dot_pairwise, dot_from_the_end, dot_tree):
                x, e, r, sft = one_step(d, b, 0.1, dot)
                assert (T.bits(e), T.bits(r), sft) == want, (name, n, dot.__name__, e, r)
                assert np.array_equal(x, x_ref) and np.array_equal(np.signbit(x), np.signbit(x_ref)), (name, n, dot.__name__)
            print("%s n = %7d: err %r rho %r soft %d — oracle, model and three summation orders agree bitwise" % (name, n, err, rho, soft))
    for n in T.DOT_SIZES:
        b, q = T.square_norm_rhs(n)
        for dot in (dot_pairwise, dot_from_the_end, dot_tree):
            assert dot(b, b) == float(q * q)
    for n in T.GS_SIZES:
        for sweeps in (1, 2):
            _, _, _, error, total = T.gs_swept(n, sweeps)
            print("B2 n = %7d, %d sweeps: oracle error %r, exact residual sum %s" % (n, sweeps, error, total))
    print("ok")


if __name__ == "__main__":
    main()
