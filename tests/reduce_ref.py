"""Python restatements of the reference's sparse-vector reductions (test infrastructure).

Every sum is a Python `for` loop over floats from 0.0 — one rounding per product and per addition, which is the arithmetic of
dot_acc (sprs/src/sparse/vec.rs:846-880), of Iterator::sum in dot_dense and the norms (vec.rs:894-958) and of
prod::csvec_dot_by_binary_search (sprs/src/sparse/prod.rs:14-70).  norm() carries the reference's branches."""
import math

import numpy as np

NONE = (1 << 64) - 1


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def chain(terms):
    """the left-to-right sum from +0.0"""
    s = 0.0
    for t in terms:
        s = s + float(t)
    return s


def reversed_chain(terms):
    return chain(list(terms)[::-1])


def pairwise_tree(terms):
    """the balanced tree: neighbours added level by level"""
    t = [float(x) for x in terms]
    if not t:
        return 0.0
    while len(t) > 1:
        t = [t[i] + t[i + 1] if i + 1 < len(t) else t[i] for i in range(0, len(t), 2)]
    return t[0]


def strided_sum(terms, lanes=64):
    """lane t adds t, t + 64, ..., then the lanes are added in order"""
    t = [float(x) for x in terms]
    return chain(chain(t[k::lanes]) for k in range(min(lanes, len(t))))


def dot_merge(vi, vd, wi, wd):
    """dot_acc's merge of two sorted sparse vectors (vec.rs:862-878)"""
    s = 0.0
    i = j = 0
    while i < len(vi) and j < len(wi):
        a, b = int(vi[i]), int(wi[j])
        if a == b:
            s = s + float(vd[i]) * float(wd[j])
        if a <= b:
            i += 1
        if a >= b:
            j += 1
    return s


def dot_by_binary_search(vi, vd, wi, wd):
    """prod::csvec_dot_by_binary_search (prod.rs:14-70): the shorter vector's entries are searched for in the other one (the
    first argument on equal counts), the matched products summed in the shorter vector's order"""
    if len(vi) > len(wi):
        vi, vd, wi, wd = wi, wd, vi, vd
    wi = np.asarray(wi, dtype=np.uint64)
    s = 0.0
    for k, x in zip(vi, vd):
        j = int(np.searchsorted(wi, np.uint64(k)))
        if j < len(wi) and int(wi[j]) == int(k):
            s = s + float(x) * float(wd[j])
    return s


def dot_dense(vi, vd, x):
    return chain(float(d) * float(x[int(i)]) for i, d in zip(vi, vd))


def squared_l2_norm(vd):
    return chain(float(d) * float(d) for d in vd)


def l2_norm(vd):
    return math.sqrt(squared_l2_norm(vd))


def l1_norm(vd):
    return chain(abs(float(d)) for d in vd)


def _fmax(a, b):
    """f64::max: the other operand when one is NaN"""
    if a != a:
        return b
    if b != b:
        return a
    return a if a > b else b


def _fmin(a, b):
    if a != a:
        return b
    if b != b:
        return a
    return a if a < b else b


def _pow(x, p):
    """powf on f64 (IEEE pow: no exceptions)"""
    try:
        return math.pow(x, p)
    except OverflowError:
        return math.inf
    except ValueError:
        return math.inf if x == 0.0 and p < 0 else math.nan


def norm(vd, p):
    """CsVec::norm (vec.rs:939-958)"""
    a = [abs(float(d)) for d in vd]
    if math.isinf(p):
        if not a:
            return 0.0
        out = -math.inf if p > 0 else math.inf
        for x in a:
            out = _fmax(out, x) if p > 0 else _fmin(out, x)
        return out
    if p == 0:
        return float(sum(1 for x in a if not x == 0.0))
    return _pow(chain(_pow(x, p) for x in a), 1.0 / p)


def unit_normalize(vd):
    """vec.rs:1051-1061 -> the new values"""
    nsq = squared_l2_norm(vd)
    if nsq > 0.0:
        n = math.sqrt(nsq)
        return np.array([float(d) / n for d in vd], dtype=np.float64)
    return np.array(vd, dtype=np.float64)


def nnz_index(vi, index):
    """vec.rs:800-805 -> position or None"""
    vi = np.asarray(vi, dtype=np.uint64)
    j = int(np.searchsorted(vi, np.uint64(index)))
    return j if j < len(vi) and int(vi[j]) == int(index) else None


# ---- inputs on which the order of a sum shows ---------------------------------------------------------------------------------

CHUNK, UNROLL, BLOCK = 64, 8, 256      # the chain's chunk, its chunks in flight and the grid stage's workgroup (csvec_reduce.hpp)
SEAMS = sorted({0, 1, CHUNK - 1, CHUNK, CHUNK + 1, CHUNK * UNROLL - 1, CHUNK * UNROLL, CHUNK * UNROLL + 1, 2 * CHUNK * UNROLL + 1,
                BLOCK - 1, BLOCK, BLOCK + 1})
# seed per seam size, chosen so that every rival order below gives other bits than the chain (tests/test_reduce_cpu.py checks it)
ORDER_SEEDS = {65: 3, 255: 9, 256: 3, 257: 3, 511: 1, 512: 1, 513: 4, 1025: 2}


def order_case(n, seed=None):
    """-> (dim, indices, data, x): n stored entries whose magnitudes spread over ~30 decimal orders (half of them within three
    orders of the largest, so that many roundings count), every fourth one the exact negative of an earlier one (and x equal at
    the two indices, so that the products cancel too)"""
    seed = ORDER_SEEDS.get(n, 1) if seed is None else seed
    rng = np.random.default_rng(seed * 100003 + n)
    dim = 3 * n + 5
    idx = np.sort(rng.choice(dim, n, replace=False)).astype(np.int64)
    expo = np.where(rng.random(n) < 0.5, rng.uniform(12.0, 15.0, n), rng.uniform(-15.0, 12.0, n))
    data = rng.standard_normal(n) * 10.0 ** expo
    x = rng.uniform(0.5, 2.0, dim) * rng.choice([-1.0, 1.0], dim)
    for j in range(3, n, 4):
        i = int(rng.integers(0, j))
        data[j] = -data[i]
        x[idx[j]] = x[idx[i]]
    return dim, idx, data, x


def order_terms(n, seed=None):
    """the term lists of the four reductions of the order test on order_case(n): dot_dense, squared_l2_norm (= dot(v, v)), l1_norm"""
    dim, idx, data, x = order_case(n, seed)
    return {"dot_dense": [float(d) * float(x[i]) for i, d in zip(idx, data)],
            "squared_l2_norm": [float(d) * float(d) for d in data],
            "l1_norm": [abs(float(d)) for d in data]}


def rivals_differ(terms):
    """the condition that keeps the order test from being vacuous: the reversed chain, a pairwise tree and the 64-way strided
    sum each give other bits than the chain"""
    want = bits(chain(terms))
    return all(bits(f(terms)) != want for f in (reversed_chain, pairwise_tree, strided_sum))
