"""numpy restatement of smmp::numeric for N = f32 (smmp.rs:151-189): the values the f32 SpGEMM must reproduce bit for bit.

The structure of the product does not depend on the values, so it is taken from the CPU oracle's f64 mul_csr_csr on the
operands cast to f64.  The values follow the reference's loop: per row of A a dense f32 workspace `tmp` is cleared on the row's
output columns (N::zero(), smmp.rs:166-170), then for each entry (k, a) of the row, in the order A stores them, every entry
(j, b) of B's row k does tmp[j] = tmp[j] + a * b (smmp.rs:174-181 over MulAcc, mul_acc.rs:28-30: multiply, then add) with
np.float32 arrays throughout — one rounding per product, one per add — and the row is read out at its sorted columns."""
import numpy as np


def as_f32(m):
    """(shape, indptr, indices, data) with the values cast to f32 (round to nearest even, as CsMat::map(|&v| v as f32))"""
    with np.errstate(over="ignore"):
        return m[0], m[1], m[2], np.asarray(m[3]).astype(np.float32)


def as_f64(m):
    return m[0], m[1], m[2], np.asarray(m[3]).astype(np.float64)


def mul_csr_csr_f32(a, b, structure=None):
    """a, b: (shape, indptr, indices, f32 data), CSR.  -> (shape, indptr, indices, f32 data) of a * b.
    structure: the f64 oracle's product of the same operands when the caller has it already."""
    if structure is None:
        from oracle import oracle
        with np.errstate(all="ignore"):
            structure = oracle.mul_csr_csr(*as_f64(a), *as_f64(b), threads=1)
    shape, c_ip, c_ix = structure[0], structure[1], structure[2]
    assert a[3].dtype == np.float32 and b[3].dtype == np.float32
    a_ip, a_ix, a_dt = a[1].astype(np.int64), a[2].astype(np.int64), a[3]
    b_ip, b_ix, b_dt = b[1].astype(np.int64), b[2].astype(np.int64), b[3]
    cp, cx = c_ip.astype(np.int64), c_ix.astype(np.int64)
    out = np.zeros(cx.size, dtype=np.float32)
    tmp = np.zeros(b[0][1], dtype=np.float32)
    with np.errstate(all="ignore"):
        for i in range(a[0][0]):
            cols = cx[cp[i]:cp[i + 1]]
            tmp[cols] = np.float32(0.0)
            for p in range(a_ip[i], a_ip[i + 1]):
                s, e = b_ip[a_ix[p]], b_ip[a_ix[p] + 1]
                j = b_ix[s:e]                                   # distinct inside one row of B: a plain fancy-index update
                tmp[j] = tmp[j] + a_dt[p] * b_dt[s:e]           # f32 * f32 -> f32, then f32 + f32 -> f32
            out[cp[i]:cp[i + 1]] = tmp[cols]
    return shape, c_ip, c_ix, out


def product_counts_and_magnitudes(a, b):
    """per output entry: the number of products that meet in it and the f64 sum of |a * b| over them (for the γ_m bounds)"""
    from oracle import oracle
    ones = lambda m: (m[0], m[1], m[2], np.ones(m[2].size))
    mags = lambda m: (m[0], m[1], m[2], np.abs(np.asarray(m[3]).astype(np.float64)))
    counts = oracle.mul_csr_csr(*ones(a), *ones(b), threads=1)[3]
    mag = oracle.mul_csr_csr(*mags(a), *mags(b), threads=1)[3]
    return np.rint(counts).astype(np.int64), mag


def gamma_bound(counts, mag):
    """γ_m Σ|a b| with m = 1 + the entry's product count, u = 2^-24 (Higham, Accuracy and Stability, eq. 3.4 for a
    recursive sum of rounded products)"""
    u = 2.0 ** -24
    m = 1.0 + counts
    return m * u / (1.0 - m * u) * mag


def same_bits(x, y):
    """bit equality of two f32 arrays where NaN equals NaN whatever its payload (x86 and gfx950 make different default NaNs)"""
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    if x.shape != y.shape:
        return False
    nx, ny = np.isnan(x), np.isnan(y)
    return bool(np.array_equal(nx, ny) and np.array_equal(x.view(np.uint32)[~nx], y.view(np.uint32)[~ny]))
