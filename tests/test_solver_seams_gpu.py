"""Seam cases of the two device-resident solver loops — BiCGSTAB (sprs_amd/csrc/bicgstab.hip) and Gauss-Seidel
(sprs_amd/csrc/gauss_seidel.hip): their reductions at the sizes where the code takes another path, and their restart branches.

The principle is the one of check_band_exact (tests/test_spmv_band_gpu.py): inputs for which every addend of every reduction is
exactly representable and every partial sum stays far below 2^53.  Every summation order then gives the same double, so the serial
oracle, the fixed tree on the device and exact integer / Fraction arithmetic written here must agree BIT FOR BIT; one stray,
stale or missing addend changes the result.  The only tolerance in this file is the 1e-10 on x of the restart cases (section C),
where the iterates are ordinary doubles.

Sizes: 2048 | 2049 is where the serial dot hands over to the tree (BICG_SERIAL_N), 8191 | 8192 | 8193 where a chunk of the tree
(DOT_CHUNK = SUM_CHUNK = 8192) holds exactly one element, 16385 two full chunks and one element, 2 097 152 | 2 097 153 = 256 | 257
chunks: the strided loop of the one-workgroup final kernels (256 threads) takes a second turn only at the last.

scripts/solver_seams_precheck.py runs the constructions of A2 / A3 on the CPU alone (oracle, and a numpy restatement under three
summation orders) and must be bitwise consistent before any of this is worth running on a device.
(Kept apart from test_gauss_seidel_gpu.py, which tests/test_emu_cpu.py runs through the CPU emulator: 2e6 rows do not belong there.)
"""
import functools
import math
import struct
from fractions import Fraction

import numpy as np
import pytest

from conftest import IDX_COMBOS
from helpers import rel_err

pytestmark = pytest.mark.gpu

DOT_SIZES = [1, 2047, 2048, 2049, 8191, 8192, 8193, 16385, 2097152, 2097153]
GS_SIZES = [1, 8191, 8192, 8193, 2097152, 2097153]
TINY_TOL = 1e-300                    # never reached: no hard restart in the one-step cases


@pytest.fixture(scope="module")
def hip():
    import sprs_amd
    if sprs_amd.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X (no CPU fallback exists)")
    return sprs_amd


def bits(v):
    """the eight bytes of a double: == on these tells +0 from -0 and never calls two different values equal"""
    return struct.pack("<d", float(v))


def exact_float(q):
    """a Fraction that must be a double"""
    v = float(q)
    assert Fraction(v) == q, "%r is not representable" % (q,)
    return v


# ---------------------------------------------------------------------------------------------------------------------------------
# constructions (pure numpy / integers: shared with scripts/solver_seams_precheck.py)
# ---------------------------------------------------------------------------------------------------------------------------------
def diag_csr(d, idx=np.uint64, ptr=np.uint64):
    """diag(d) as CSR (== CSC) arrays: one entry per row, so the SpMV is a single product per row and exact"""
    n = d.size
    return np.arange(n + 1, dtype=ptr), np.arange(n, dtype=idx), np.ascontiguousarray(d, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def square_norm_rhs(n, seed=7):
    """A1: b in +-{1, 2, 3}, no zero, with sum b^2 = q^2 a perfect square (so sqrt and err * err round-trip): n1 ones, n2 twos
    and n3 threes with n1 + 4 n2 + 9 n3 = q^2, i.e. 3 n2 + 8 n3 = q^2 - n, about a third of each, in a seeded order.
    Every element adds at least 1 to the sum: a dropped or doubled one is seen.  Returns (b, q)."""
    for q in range(math.isqrt(14 * n // 3), 0, -1):
        left = q * q - n
        if left < 0:
            break
        for n3 in range(min(n // 3, left // 8), max(min(n // 3, left // 8) - 3, -1), -1):
            n2, rem = divmod(left - 8 * n3, 3)
            if rem == 0 and n2 + n3 <= n:
                rng = np.random.default_rng(seed + n)
                mag = np.repeat([1.0, 2.0, 3.0], [n - n2 - n3, n2, n3])
                b = rng.permutation(mag) * rng.choice([-1.0, 1.0], size=n)
                assert int((b * b).sum()) == q * q and np.all(b != 0.0)
                return b, q
    raise AssertionError("no composition for n = %d" % n)


STEP_PLAIN = ((1, 3, 5), (9, 6, 1))       # A2: alpha = 1/2, omega = 1/4, rho / err^2 = 2: no soft restart
STEP_SOFT = ((1, 3, -3), (1, 1, 3))       # A3: alpha = -1, omega = 1/16, |rho| / err^2 = 2/31 < 0.1: soft restart


@functools.lru_cache(maxsize=None)
def class_system(n, spec, seed=11):
    """A2 / A3: a diagonal matrix with the three diagonal values `d` of spec = (d, w), and b in +-{1, 2, 3} such that class c
    carries sum b^2 = w_c u.  With x0 = 0 every scalar of the first step then depends on d and w alone, and sum b^2 = W u
    (W = sum w) must be a perfect square q^2: err = sqrt(sum b^2) and rho = err * err round-trip, alpha stays dyadic.
    (Without that condition alpha comes out as 0.5000000000000001 and the step depends on the order of the additions.)
    Start from w_c u elements of b = 1 per class; four b = 1 of one class may be replaced by one b = 2 (3 elements fewer) and nine
    by one b = 3 (8 fewer): n = q^2 - 3 j - 8 m.  The classes lie over the positions in a seeded permutation, signs are random,
    b != 0 everywhere — in the last 256 positions and around the multiples of 8192 like anywhere else.
    Returns (dvals, b, class sums of b^2); n must be at least 3."""
    d, w = spec
    W = sum(w)
    for q in range(math.isqrt(n - 1) + 1, 2 * math.isqrt(n) + 64):
        if (q * q) % W:
            continue
        u = q * q // W
        for m in range(0, (q * q - n) // 8 + 1):
            j, rem = divmod(q * q - n - 8 * m, 3)
            if rem:
                continue
            ones, twos, threes, jl, ml = [wc * u for wc in w], [0, 0, 0], [0, 0, 0], j, m
            for c in sorted(range(3), key=lambda c: -ones[c]):
                threes[c] = min(ml, ones[c] // 9)
                ml -= threes[c]
                ones[c] -= 9 * threes[c]
                twos[c] = min(jl, ones[c] // 4)
                jl -= twos[c]
                ones[c] -= 4 * twos[c]
            if jl or ml:
                continue
            rng = np.random.default_rng(seed + n)
            mag = np.concatenate([np.repeat([1.0, 2.0, 3.0], [ones[c], twos[c], threes[c]]) for c in range(3)])
            cls = np.concatenate([np.full(ones[c] + twos[c] + threes[c], c) for c in range(3)])
            assert mag.size == n
            perm = rng.permutation(n)
            mag, cls = mag[perm], cls[perm]
            b = mag * rng.choice([-1.0, 1.0], size=n)
            sums = tuple(int((mag[cls == c] ** 2).sum()) for c in range(3))
            assert sums == tuple(wc * u for wc in w) and np.all(b != 0.0)
            return np.asarray(d, dtype=np.float64)[cls], b, sums
    raise AssertionError("no composition for n = %d" % n)


def step_model(spec, sums, thr):
    """ONE step() of bicgstab.rs:194-229 after new() with x0 = 0 on a class system, in exact arithmetic.  Every vector of the step
    is (a coefficient per class) * b, every dot a combination of the class sums.  Returns what the solver must hold after the
    step: the per-class coefficient of x, err, rho, soft_restart_count."""
    d = [Fraction(v) for v in spec[0]]
    S = [Fraction(v) for v in sums]
    dot = lambda f, g: sum(fc * gc * sc for fc, gc, sc in zip(f, g, S))
    one = [Fraction(1)] * 3
    rr = dot(one, one)                                        # r = rhat = p = b
    q = math.isqrt(int(rr))
    assert q * q == rr                                        # err = sqrt(rr) and rho = err * err are exact
    alpha = rr / dot(one, d)                                  # v = A p = d b
    s = [1 - alpha * dc for dc in d]
    t = [dc * sc for dc, sc in zip(d, s)]
    omega = dot(t, s) / dot(t, t)
    x = [alpha + omega * sc for sc in s]                      # h = p alpha, x = h + omega s
    r = [sc - omega * tc for sc, tc in zip(s, t)]
    err2, rho = dot(r, r), dot(one, r)
    err = math.sqrt(exact_float(err2))
    soft = abs(exact_float(rho)) / (err * err) < thr
    for v in [alpha, omega] + s + t + x + r + ([] if soft else [rho / rr, alpha / omega]):      # (the last two make beta)
        exact_float(v)                                        # every scalar and coefficient of the step is a double ...
        assert v.denominator <= 64                            # ... with at most six fractional bits
    return [exact_float(v) for v in x], err, (err * err if soft else exact_float(rho)), int(soft)


@functools.lru_cache(maxsize=None)
def gs_block_system(n, seed=5):
    """B: rows in blocks of 8.  The diagonal is 2 or 4, row i has an entry +-1 at i - 1 except at a block's first row and an
    entry +-1 at i + 1 except at a block's last row (columns ascending inside a row); x0 and rhs are integers in +-{1, 2, 3}.
    Returns (indptr, indices, data, x0, rhs, (lo, diag, up) as dense vectors, 0 where there is no entry)."""
    rng = np.random.default_rng(seed + n)
    i = np.arange(n)
    has_lo = (i % 8) != 0
    has_up = ((i % 8) != 7) & (i != n - 1)
    diag = rng.choice([2.0, 4.0], size=n)
    lo = np.where(has_lo, rng.choice([-1.0, 1.0], size=n), 0.0)
    up = np.where(has_up, rng.choice([-1.0, 1.0], size=n), 0.0)
    ip = np.zeros(n + 1, dtype=np.uint64)
    ip[1:] = np.cumsum(1 + has_lo.astype(np.int64) + has_up.astype(np.int64))
    start = ip[:-1].astype(np.int64)
    ix = np.zeros(int(ip[-1]), dtype=np.uint64)
    dt = np.zeros(int(ip[-1]))
    ix[start[has_lo]], dt[start[has_lo]] = i[has_lo] - 1, lo[has_lo]
    at = start + has_lo
    ix[at], dt[at] = i, diag
    at = (start + has_lo + 1)[has_up]
    ix[at], dt[at] = i[has_up] + 1, up[has_up]
    x0 = rng.integers(1, 4, size=n) * rng.choice([-1.0, 1.0], size=n)
    rhs = rng.integers(1, 4, size=n) * rng.choice([-1.0, 1.0], size=n)
    return ip, ix, dt, x0, rhs, (lo, diag, up)


def block_matvec(bands, x):
    """A x of a gs_block_system, for values that make every product and sum exact"""
    lo, diag, up = bands
    v = diag * x
    v[1:] += lo[1:] * x[:-1]
    v[:-1] += up[:-1] * x[1:]
    return v


# B2.  Bound on the iterates: a row divides by at most 4 = 2^2, so a sweep adds at most 2 fractional bits per row of a chain, and
# a chain is a block of 8 rows: 16 bits in the first sweep (row i of a block: 2 (i + 1)); in the second, row i reads its new left
# neighbour and the OLD right one (2 (i + 2) bits): 2 i + 6, and 20 for a block's last row.  Magnitudes: |x0|, |rhs| <= 3,
# off-diagonals +-1, diagonal >= 2: |x_i| <= (3 + |x_{i-1}| + max|x_old|) / 2, below 6 after one sweep and below 9 after two.
# So x 2^20 is an integer below 2^24.  Row i has just been solved with the old x_{i+1}, hence
# v_i - rhs_i = up_i (x_new_{i+1} - x_old_{i+1}): below 2^4 in magnitude, 20 fractional bits, and the sum over 2^21 + 1 rows stays
# below 2^(4 + 22 + 20) = 2^46 units of 2^-20: every partial sum of every order is exact.
GS_FRAC_BITS, GS_MAX_ABS = 20, 9.0


@functools.lru_cache(maxsize=None)
def gs_swept(n, sweeps):
    """the oracle's iterate after `sweeps` sweeps of gs_block_system(n), with the SIGN of (x0, rhs) chosen so that the signed
    residual sum is positive (the system is linear: flipping both flips every iterate and the sum exactly; a negative sum would
    make `error` a NaN, which compares nothing).  Returns (x0, rhs, x_ref, error_ref, exact residual sum as a Fraction)."""
    from oracle import oracle
    ip, ix, dt, x0, rhs, bands = gs_block_system(n)
    for sign in (1.0, -1.0):
        x_ref, info = oracle.gauss_seidel((n, n), ip, ix, dt, sign * x0, sign * rhs, sweeps, -1.0)
        scaled = x_ref * 2.0 ** GS_FRAC_BITS
        assert np.array_equal(scaled, np.rint(scaled)) and np.abs(x_ref).max() < GS_MAX_ABS      # the bound stated above
        resid = (block_matvec(bands, x_ref) - sign * rhs) * 2.0 ** GS_FRAC_BITS
        assert np.array_equal(resid, np.rint(resid)) and np.abs(resid).max() < 2.0 ** (4 + GS_FRAC_BITS)
        total = Fraction(int(resid.astype(np.int64).sum()), 2 ** GS_FRAC_BITS)                  # integer sum: exact
        if total > 0 or n == 1:                          # (a single row is solved exactly: its residual is 0)
            assert info["converged"] == 0 and info["iterations"] == sweeps
            return sign * x0, sign * rhs, x_ref, info["error"], total
    raise AssertionError("residual sum is zero for n = %d" % n)


# ---------------------------------------------------------------------------------------------------------------------------------
# device front ends
# ---------------------------------------------------------------------------------------------------------------------------------
def bicg_gpu(n, ip, ix, dt, x0, b, tol, max_iter, thr=0.1, storage="CSR", stream=None):
    from sprs_amd.device import DeviceCsMat, DeviceVec, CSR, CSC
    from sprs_amd.linalg import BiCGSTAB
    a = DeviceCsMat.from_host((n, n), ip, ix, dt, storage=CSR if storage == "CSR" else CSC)
    return BiCGSTAB.solve(a, DeviceVec.from_host(x0), DeviceVec.from_host(b), tol, max_iter, thr, stream=stream)


def gs_gpu(n, ip, ix, dt, x0, rhs, max_iter, eps, stream=None):
    from sprs_amd.device import DeviceCsMat, DeviceVec
    from sprs_amd.linalg import gauss_seidel
    a = DeviceCsMat.from_host((n, n), ip, ix, dt)
    x = DeviceVec.from_host(x0)
    res = gauss_seidel(a, x, DeviceVec.from_host(rhs), max_iter, eps, stream=stream)
    return x.to_host(), res


def counts(res):
    return res.iteration_count(), res.soft_restart_count(), res.hard_restart_count(), res.converged


def info_counts(info):
    return info["iteration_count"], info["soft_restart_count"], info["hard_restart_count"], bool(info["converged"])


# ---------------------------------------------------------------------------------------------------------------------------------
# A. BiCGSTAB dots at their seams
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", DOT_SIZES)
def test_initial_norm_is_exact(hip, n):
    """A1 — the single-pair dot (c == NULL) of new(): max_iter = 0, x0 = 0, sum b^2 = q^2: err == q and rho == q^2 to the bit, on
    the device, in the oracle and in integers; nothing else happens"""
    from oracle import oracle
    b, q = square_norm_rhs(n)
    ip, ix, dt = diag_csr(np.resize([1.0, 3.0, 5.0], n))
    x0 = np.zeros(n)
    x_ref, info = oracle.bicgstab((n, n), ip, ix, dt, x0, b, 1e-9, 0)
    assert (bits(info["err"]), bits(info["rho"])) == (bits(q), bits(q * q)) and info_counts(info) == (0, 0, 0, False)
    assert np.array_equal(x_ref, x0)
    res = bicg_gpu(n, ip, ix, dt, x0, b, 1e-9, 0)
    print("n = %d: err %r (q = %d), rho %r" % (n, res.err(), q, res.rho()))
    assert bits(res.err()) == bits(q)
    assert bits(res.rho()) == bits(q * q)
    assert counts(res) == (0, 0, 0, False)
    assert np.array_equal(res.x().to_host(), x0)


def check_one_step(n, spec, soft_expected, idx=np.uint64, ptr=np.uint64, storage="CSR"):
    """A2 / A3: max_iter = 1 from x0 = 0 on class_system(n, spec): both two-pair dots and both of their outputs enter x, err
    and rho; device == oracle == the Fraction model, bit for bit"""
    from oracle import oracle
    d, b, sums = class_system(n, spec)
    ip, ix, dt = diag_csr(d, idx, ptr)
    x0 = np.zeros(n)
    xc, err, rho, soft = step_model(spec, sums, 0.1)
    assert soft == soft_expected
    x_model = np.zeros(n)
    for dv, xv in zip(spec[0], xc):
        x_model[d == dv] = xv * b[d == dv]                                 # a dyadic coefficient times a small integer: exact
    x_ref, info = oracle.bicgstab((n, n), ip, ix, dt, x0, b, TINY_TOL, 1, storage=storage)
    assert np.array_equal(x_ref, x_model)                                  # the reference alone is already order-independent here
    assert (bits(info["err"]), bits(info["rho"])) == (bits(err), bits(rho))
    assert info_counts(info) == (1, soft, 0, False)
    res = bicg_gpu(n, ip, ix, dt, x0, b, TINY_TOL, 1, storage=storage)
    print("n = %d: err %r (model %r), rho %r (model %r), counts %r" % (n, res.err(), err, res.rho(), rho, counts(res)))
    assert counts(res) == (1, soft, 0, False)
    assert bits(res.err()) == bits(err)
    assert bits(res.rho()) == bits(rho)
    x = res.x().to_host()
    assert np.array_equal(x, x_ref) and np.array_equal(np.signbit(x), np.signbit(x_ref))
    return x, res


def check_one_element_breakdown(spec):
    """n = 1 admits no three classes.  The one-element system is the reference's breakdown instead (the half step solves it, s = 0,
    omega = 0 / 0: bicgstab.rs:206): NaN everywhere, in the oracle and on the device alike, and no restart is counted"""
    from oracle import oracle
    ip, ix, dt = diag_csr(np.array([float(spec[0][2])]))
    x_ref, info = oracle.bicgstab((1, 1), ip, ix, dt, np.zeros(1), np.ones(1), TINY_TOL, 1)
    res = bicg_gpu(1, ip, ix, dt, np.zeros(1), np.ones(1), TINY_TOL, 1)
    assert np.isnan(x_ref).all() and np.isnan(info["err"]) and np.isnan(info["rho"])
    assert np.isnan(res.x().to_host()).all() and np.isnan(res.err()) and np.isnan(res.rho())
    assert counts(res) == info_counts(info) == (1, 0, 0, False)


@pytest.mark.parametrize("n", DOT_SIZES)
def test_one_step_with_exact_dots(hip, n):
    """A2 — d = (1, 3, 5) carrying sum b^2 as 9 : 6 : 1: alpha = 1/2, omega = 1/4, r = (3/8, -1/8, 3/8) b, rho / err^2 = 2"""
    if n == 1:
        check_one_element_breakdown(STEP_PLAIN)
    else:
        check_one_step(n, STEP_PLAIN, 0)


@pytest.mark.parametrize("n", DOT_SIZES)
def test_one_step_through_the_soft_restart(hip, n):
    """A3 — d = (1, 3, -3) carrying sum b^2 as 1 : 1 : 3: alpha = -1, omega = 1/16, |rho| / err^2 = 2/31 < 0.1: the step ends in
    soft_restart(), rho = err * err as the solver computes it"""
    if n == 1:
        check_one_element_breakdown(STEP_SOFT)
    else:
        x, res = check_one_step(n, STEP_SOFT, 1)
        assert res.soft_restart_count() == 1 and bits(res.rho()) == bits(res.err() * res.err())


@pytest.mark.parametrize("idx,ptr", IDX_COMBOS)
def test_one_step_index_widths(hip, idx, ptr):
    check_one_step(8193, STEP_PLAIN, 0, idx, ptr)


def test_one_step_csc_operand(hip):
    """the matrix uploaded as CSC: converted once on the device (to_other_storage) before the loop"""
    check_one_step(8193, STEP_PLAIN, 0, storage="CSC")


# ---------------------------------------------------------------------------------------------------------------------------------
# B. Gauss-Seidel's residual sum at its seams
# ---------------------------------------------------------------------------------------------------------------------------------
def check_zero_sweeps(n, sign):
    from oracle import oracle
    ip, ix, dt, x0, _, bands = gs_block_system(n)
    c = np.resize([1.0, 3.0, 2.0, 1.0, 2.0], n) * sign             # v_i - rhs_i = c_i: nonzero in every row
    rhs = block_matvec(bands, x0) - c                               # small integers
    total = int(c.sum())
    expected = math.sqrt(total) if total >= 0 else math.nan
    x_ref, info = oracle.gauss_seidel((n, n), ip, ix, dt, x0, rhs, 0, 1e-8)
    x, res = gs_gpu(n, ip, ix, dt, x0, rhs, 0, 1e-8)
    print("n = %d: error %r, oracle %r, sqrt(%d) = %r" % (n, res.error, info["error"], total, expected))
    assert np.array_equal(x, x0) and np.array_equal(x_ref, x0)
    assert (res.converged, res.iterations) == (False, 0) == (bool(info["converged"]), info["iterations"])
    if total < 0:
        assert np.isnan(info["error"]) and np.isnan(res.error)
    else:
        assert bits(info["error"]) == bits(expected)
        assert bits(res.error) == bits(expected)


@pytest.mark.parametrize("n", GS_SIZES)
def test_zero_sweeps_error_is_exact(hip, n):
    """B1 — max_iter = 0: error = sqrt(sum (v_i - rhs_i)) of the start vector, an exact integer sum; x untouched"""
    check_zero_sweeps(n, 1.0)


def test_zero_sweeps_negative_sum_is_nan(hip):
    """B1 — the SIGNED sum, as the reference has it: negative gives NaN (heat.rs:111)"""
    check_zero_sweeps(8193, -1.0)


@pytest.mark.parametrize("sweeps", [1, 2])
@pytest.mark.parametrize("n", GS_SIZES)
def test_sweeps_with_exact_iterates(hip, n, sweeps):
    """B2 — one and two sweeps of gs_block_system: every iterate is a dyadic rational (bound above gs_swept), so `error` is pinned
    to the bit as well — against the oracle and against the integer sum of the residual"""
    ip, ix, dt, _, _, _ = gs_block_system(n)
    x0, rhs, x_ref, error_ref, total = gs_swept(n, sweeps)
    expected = math.sqrt(exact_float(total))
    assert bits(error_ref) == bits(expected) and (expected > 0.0 or n == 1)
    x, res = gs_gpu(n, ip, ix, dt, x0, rhs, sweeps, -1.0)
    print("n = %d, %d sweeps: error %r, oracle %r, exact sum %r" % (n, sweeps, res.error, error_ref, total))
    assert np.array_equal(x, x_ref)
    assert bits(res.error) == bits(expected)
    assert (res.converged, res.iterations) == (False, sweeps)
    assert res.levels == min(8, n)


def test_sweep_redraws(hip):
    """B3 — the sweep launches at most one workgroup per CU and its waves draw 64 positions of the level order at a time: with
    more rows than 256 x CUs every wave draws again and again (2 097 153 rows: 32 769 draws)"""
    import torch
    n = 2097153
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert hip.get_option("gauss_seidel_blocks") == 0 and n > 256 * cus, "the grid covers the system: nothing is redrawn"
    ip, ix, dt, _, _, _ = gs_block_system(n)
    x0, rhs, x_ref, error_ref, _ = gs_swept(n, 2)
    x, res = gs_gpu(n, ip, ix, dt, x0, rhs, 2, -1.0)
    assert np.array_equal(x, x_ref) and bits(res.error) == bits(error_ref)


# ---------------------------------------------------------------------------------------------------------------------------------
# C. restart logic against the oracle in the serial range (n <= 2048)
# ---------------------------------------------------------------------------------------------------------------------------------
def serial_system():
    from test_bicgstab_gpu import _diag_dominant
    n = 1500
    a = _diag_dominant(n, 3)
    rng = np.random.default_rng(1)
    return n, a.indptr.astype(np.uint64), a.indices.astype(np.uint64), a.data, rng.standard_normal(n), rng.standard_normal(n)


def check_tracks_oracle(res, x_ref, info):
    assert counts(res) == info_counts(info)
    assert rel_err(res.x().to_host(), x_ref) <= 1e-10


def test_every_step_soft_restarts(hip):
    """soft_restart_threshold = 1e300: |rho| / err^2 is below it in every step"""
    from oracle import oracle
    n, ip, ix, dt, x0, b = serial_system()
    x_ref, info = oracle.bicgstab((n, n), ip, ix, dt, x0, b, 1e-10, 60, soft_restart_threshold=1e300)
    assert info["soft_restart_count"] == info["iteration_count"] >= 5 and info["converged"] == 1
    res = bicg_gpu(n, ip, ix, dt, x0, b, 1e-10, 60, thr=1e300)
    assert res.soft_restart_count() == res.iteration_count()
    check_tracks_oracle(res, x_ref, info)


def test_never_a_soft_restart(hip):
    """soft_restart_threshold = 0: nothing is below it"""
    from oracle import oracle
    n, ip, ix, dt, x0, b = serial_system()
    x_ref, info = oracle.bicgstab((n, n), ip, ix, dt, x0, b, 1e-10, 60, soft_restart_threshold=0.0)
    assert info["soft_restart_count"] == 0 and info["iteration_count"] >= 5 and info["converged"] == 1
    res = bicg_gpu(n, ip, ix, dt, x0, b, 1e-10, 60, thr=0.0)
    assert res.soft_restart_count() == 0
    check_tracks_oracle(res, x_ref, info)


@pytest.mark.parametrize("thr", [0.1, 0.0])
def test_hard_restarts_that_do_not_confirm(hip, golden, thr):
    """the reference's own 4 x 4 system at tol 1e-60 (bicgstab.rs:336-369): twice the running estimate passes tol, hard_restart()
    recomputes the true residual, finds it above tol and the iteration goes on from the restarted directions; the third time the
    residual is exactly zero.  The oracle's counts are asserted first: the case must keep covering the branch."""
    from oracle import oracle
    fx = golden["bicgstab_example"]
    ip, ix = np.array(fx["indptr"], dtype=np.uint64), np.array(fx["indices"], dtype=np.uint64)
    dt = np.array(fx["data"])
    x_ref, info = oracle.bicgstab((4, 4), ip, ix, dt, np.ones(4), np.ones(4), fx["tol"], fx["max_iter"], thr, storage="CSC")
    assert info_counts(info) == (45, 0, 3, True)
    res = bicg_gpu(4, ip, ix, dt, np.ones(4), np.ones(4), fx["tol"], fx["max_iter"], thr=thr, storage="CSC")
    assert res.hard_restart_count() >= 2
    assert counts(res) == info_counts(info)
    assert np.array_equal(res.x().to_host(), x_ref) and bits(res.err()) == bits(info["err"]) == bits(0.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# D. streams, and the empty system
# ---------------------------------------------------------------------------------------------------------------------------------
def test_solvers_on_a_nonblocking_stream(hip):
    """D1 — both solvers read scalars back in every iteration, on the caller's stream: on a torch stream (hipStreamNonBlocking: not
    ordered with the null stream) they give the bits of the null stream.  The A2 step at 16385 (three chunks), then four more
    steps of it; two sweeps of the B2 system at 8193."""
    import torch
    s = torch.cuda.Stream(device=torch.device("cuda", 0))
    n = 16385
    d, b, _ = class_system(n, STEP_PLAIN)
    ip, ix, dt = diag_csr(d)
    for max_iter in (1, 5):
        out = []
        for stream in (s.cuda_stream, None):
            res = bicg_gpu(n, ip, ix, dt, np.zeros(n), b, TINY_TOL, max_iter, stream=stream)
            out.append((res.x().to_host().tobytes(), bits(res.err()), bits(res.rho()), counts(res)))
        assert out[0] == out[1]
    x1, _ = check_one_step(n, STEP_PLAIN, 0)
    res = bicg_gpu(n, ip, ix, dt, np.zeros(n), b, TINY_TOL, 1, stream=s.cuda_stream)
    assert np.array_equal(res.x().to_host(), x1)
    n = 8193
    ip, ix, dt, _, _, _ = gs_block_system(n)
    x0, rhs, x_ref, error_ref, _ = gs_swept(n, 2)
    x_s, res_s = gs_gpu(n, ip, ix, dt, x0, rhs, 2, -1.0, stream=s.cuda_stream)
    x_0, res_0 = gs_gpu(n, ip, ix, dt, x0, rhs, 2, -1.0)
    assert np.array_equal(x_s, x_0) and np.array_equal(x_s, x_ref)
    assert bits(res_s.error) == bits(res_0.error) == bits(error_ref)


@pytest.mark.parametrize("max_iter,tol,expected", [(0, 1e-9, (0, 0, 0, False)), (3, 1e-9, (1, 0, 1, True)), (3, 0.0, (3, 0, 0, False))])
def test_empty_system(hip, max_iter, tol, expected):
    """D2 — n = 0 as the reference's solve() (bicgstab.rs:148-171) has it, the oracle being the judge: without an iteration the
    loop falls through to Err; otherwise the first step's err = sqrt(0) = 0 passes any tol > 0, the hard restart confirms it and
    solve() returns Ok after one iteration with one hard restart; with tol = 0 nothing is below it and the iterations run out"""
    from oracle import oracle
    ip, ix, z = np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint64), np.zeros(0)
    x_ref, info = oracle.bicgstab((0, 0), ip, ix, z, z, z, tol, max_iter)
    assert info_counts(info) == expected and (bits(info["err"]), bits(info["rho"])) == (bits(0.0), bits(0.0))
    res = bicg_gpu(0, ip, ix, z, z, z, tol, max_iter)
    assert counts(res) == expected
    assert (bits(res.err()), bits(res.rho())) == (bits(0.0), bits(0.0))
    assert res.x().to_host().size == 0
