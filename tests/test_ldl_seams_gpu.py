"""Device LDL^T at the seams the feature tests (tests/test_ldl_gpu.py) do not reach on a real chip: a wave's second and third row
(the flag words of the pattern pass, the cleared y, the carried cursor and spin count), a row of exactly ldl_lds_cap and of
ldl_lds_cap + 1 entries, the second launch of the elimination-tree kernel, the clamp of the flag words to 1 GiB, the solves'
second chunk, two zero pivots far apart, and the NaN whose bits are the "pending" tag.  Every comparison is exact: integers, or
the bits of f64 values against the restatement tests/ldl_ref.py; where the restatement has NaNs, their positions and every other
bit.

All shapes derive from the chip: the pattern and the numeric kernel launch 2 x CUs workgroups of 4 waves, WAVES = 8 x CUs.  Each
test first asserts the condition that makes it meaningful.  The matrices are built sparsely: a symmetric, strictly diagonally
dominant tridiagonal core (parent(i) = i + 1) plus long-range entries (r, c), which make row r of L the dense run c .. r - 1.

The cases not marked "real device only" also run against the kernel emulator (tests/test_ldl_emu_cpu.py), which reports 4 CUs."""
import numpy as np
import pytest

import ldl_ref as R
from conftest import IDX_COMBOS
from test_ldl_gpu import CSC, CSR, EMULATED, _default_options, _mat, _need_device, _perm, _rhs, _same_bits, _same_factors  # noqa: F401

pytestmark = pytest.mark.gpu

CAPS = (1024, 8)                                            # the option's default, and the small cap of the feature tests
ALL_ONES = np.frombuffer(np.uint64(0xFFFFFFFFFFFFFFFF).tobytes(), dtype=np.float64)[0]


def _cus():
    if EMULATED:
        return 4                                            # tests/emu/hip/hip_runtime.h
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- generators ----------------------------------------------------------------------------------------------------------------

def chain_matrix(n, longs, seed, cuts=(), ones=()):
    """Symmetric CSR (== its CSC) with a full stored diagonal: the links (i + 1, i) except where i is in `cuts`, the entries
    `longs`, off-diagonal values with many mantissa bits, the diagonal above the row's absolute sum.  `ones`: rows whose stored
    values are all 1.0 (the 2 x 2 blocks [[1, 1], [1, 1]] of the zero-pivot case)."""
    rng = np.random.RandomState(seed)
    rows = [dict() for _ in range(n)]
    pairs = [(i + 1, i) for i in range(n - 1) if i not in cuts] + sorted(set(longs))
    for (r, c), v in zip(pairs, rng.standard_normal(len(pairs)) * 3.0):
        assert 0 <= c < r < n
        rows[r][c] = rows[c][r] = 1.0 if r in ones else float(v)
    extra = rng.rand(n) + 0.5
    indptr, indices, data = [0], [], []
    for r in range(n):
        rows[r][r] = 1.0 if r in ones else sum(abs(v) for v in rows[r].values()) + float(extra[r])
        for c in sorted(rows[r]):
            indices.append(c)
            data.append(rows[r][c])
        indptr.append(len(indices))
    return n, np.array(indptr, dtype=np.uint64), np.array(indices, dtype=np.uint64), np.array(data, dtype=np.float64)


def rescaled(m, seed):
    """the pattern of m with other values: every off-diagonal pair times one factor in [1, 1.25), the diagonal times one in
    [1.25, 1.5), so the matrix stays symmetric and strictly diagonally dominant"""
    n, ip, ix, dt = m
    rng = np.random.RandomState(seed)
    factor = {}
    out = np.array(dt, dtype=np.float64)
    for r in range(n):
        for p in range(int(ip[r]), int(ip[r + 1])):
            c = int(ix[p])
            key = (min(r, c), max(r, c))
            if key not in factor:
                factor[key] = (1.25 if r == c else 1.0) + 0.25 * rng.rand()
            out[p] = dt[p] * factor[key]
    return n, ip, ix, out


def seam_longs(n, waves):
    """The long-range entries of the rows-per-wave case (identity order: entry (r, c) = a row of r - c entries)."""
    longs = [(20, 10), (20 + waves, 15),                    # rows k and k + WAVES of one wave: nodes 15 .. 19 are in both patterns
             (2 * waves + 1, waves - 3)]                    # the third row of wave 1 passes node WAVES, which its second row claimed
    for cap in CAPS:                                        # a row of exactly cap and one of cap + 1 entries, where they fit
        if cap + 8 < n:
            longs += [(cap + 6, 6), (cap + 7, 6)]
    if n >= 1000:                                           # a column with more than 64 entries under a row of more than 128
        longs += [(302 + t, 300) for t in range(70)] + [(700, 300)]
    return longs


def block_matrix(n, seed, block=97):
    """Independent diagonal blocks of `block` rows, tridiagonal inside a block, plus (r, r - 4) on every third row: short
    dependency chains at any n"""
    cuts = set(range(block - 1, n, block))
    longs = [(r, r - 4) for r in range(0, n, 3) if r % block >= 4]
    return chain_matrix(n, longs, seed, cuts)


def interleave(n):
    return list(range(0, n, 2)) + list(range(1, n, 2))


# ---- the reference, once per input -----------------------------------------------------------------------------------------------

_REFS = {}


def _ref(name, make, perm):
    """(matrix, restatement's factors, rhs, restatement's solution) of a named input under a permutation: computed once"""
    key = (name, None if perm is None else tuple(perm))
    if key not in _REFS:
        m = make()
        ref = R.factor(*m, perm)
        b = _rhs(m[0], 5)
        want, _ = R.solve(m[0], ref[1], ref[2], ref[3], ref[4], perm, b)
        _REFS[key] = (m, ref, b, want)
    return _REFS[key]


def _device_check(m, ref, b, want, perm=None, storage=CSC, idx=np.uint64, ptr=np.uint64, cap=None):
    import sprs_amd
    from sprs_amd import LdlSymbolic
    from sprs_amd.device import DeviceVec
    if cap is not None:
        sprs_amd.set_option("ldl_lds_cap", cap)
    a = _mat(m, storage, idx, ptr)
    sym = LdlSymbolic.new_perm(a, _perm(perm, idx), True)
    assert sym.parents() == ref[0] and sym.colptr().tolist() == ref[1]   # (before the numeric pass runs on a wrong pattern)
    num = sym.factor(a)
    _same_factors(sym, num, ref)
    assert _same_bits(num.solve(DeviceVec.from_host(b)).to_host(), want)
    return sym, num, a


# ---- 1. rows per wave, flag-word reuse, both homes of y ------------------------------------------------------------------------

def _seam_case():
    waves = 8 * _cus()
    n = 2 * waves + 3
    return waves, n, lambda: chain_matrix(n, seam_longs(n, waves), 4100)


def _seam_perms(n):
    return {"identity": None, "reversal": list(range(n - 1, -1, -1)), "interleave": interleave(n)}


def test_seam_matrix_reaches_the_seams():
    """the conditions of the rows-per-wave case, from the restatement alone (nothing here touches the device)"""
    import sprs_amd
    waves, n, make = _seam_case()
    assert n > 2 * waves, "every wave of the pattern pass has one row: nothing is reused"
    m, ref, _, _ = _ref("seam", make, None)
    for perm in _seam_perms(n).values():
        parents, _, colptr = R.symbolic(m[0], m[1], m[2], perm)
        assert colptr[n] <= 64 * n, "nnz(L) = %d: the restatement would take too long" % colptr[n]
    rows = R.row_patterns(m[0], m[1], m[2], None, ref[0])
    # (a) two rows of ONE wave (k and k + WAVES, k + WAVES and k + 2 WAVES) whose patterns share nodes
    assert set(rows[20]) & set(rows[20 + waves]) and set(rows[1 + waves]) & set(rows[1 + 2 * waves])
    lengths = [len(r) for r in rows]
    assert sprs_amd.get_option("ldl_lds_cap") == CAPS[0]
    for cap in CAPS:                                        # (b)
        if cap + 8 < n:
            assert lengths.count(cap) >= 1 and lengths.count(cap + 1) >= 1
    assert any(cap + 8 < n for cap in CAPS)
    if not EMULATED:                                        # (c) the 64-lane strides loop: needs more rows than the emulator's 67
        assert CAPS[0] + 8 < n, "no row reaches the default cap on this chip"
        below = [0] * n
        hit = False
        for k in range(n):
            hit = hit or (lengths[k] > 128 and any(below[i] > 64 for i in rows[k]))
            for i in rows[k]:
                below[i] += 1
        assert hit, "no row of more than 128 entries meets a column with more than 64 earlier entries"


def _seam_params():
    out = []
    for name in ("identity", "reversal", "interleave"):
        for storage in (CSR, CSC):
            for cap in CAPS:
                out.append(pytest.param(name, storage, np.uint64, np.uint64, cap, id="%s-%s-u64-u64-cap%d" % (name, ("csr", "csc")[storage], cap)))
    for idx, ptr in IDX_COMBOS[1:]:                         # (the first combination is the one above)
        for storage, cap in ((CSR, CAPS[0]), (CSC, CAPS[1])):
            out.append(pytest.param("identity", storage, idx, ptr, cap,
                                    id="identity-%s-%s-%s-cap%d" % (("csr", "csc")[storage], np.dtype(idx).name, np.dtype(ptr).name, cap)))
    return out


@pytest.mark.parametrize("name,storage,idx,ptr,cap", _seam_params())
def test_rows_per_wave(name, storage, idx, ptr, cap):
    waves, n, make = _seam_case()
    assert n > 2 * waves
    perm = _seam_perms(n)[name]
    m, ref, b, want = _ref("seam", make, perm)
    assert ref[1][n] <= 64 * n
    _device_check(m, ref, b, want, perm, storage, idx, ptr, cap)


def test_last_row_ends_the_scratch():
    """a row that keeps y in device memory owns scratch[rowptr[k] .. rowptr[k + 1]).  Here it is the last row, its slice ends the
    array, and nnz(L) < k + its length: any other offset (the row number, say) leaves the array, which the emulator's guard page
    behind every allocation turns into a fault.  (On the emulator ONE wave factors every row, since a wave that never waits
    never yields, so two rows cannot meet in a shared slice there; on the device the rows-per-wave case has them in flight
    together.)"""
    n, cap = 40, 8
    m, ref, b, want = _ref("tail", lambda: chain_matrix(n, [(n - 1, 10)], 40, cuts={0, 1, 2, 3}), None)
    colptr = ref[1]
    length = sum(1 for r in ref[2] if r == n - 1)
    assert length == n - 1 - 10 and length > cap and n - 1 + length >= colptr[n] + 4
    _device_check(m, ref, b, want, cap=cap)


# ---- 2. the second launch of the elimination-tree kernel -----------------------------------------------------------------------

@pytest.mark.skipif(EMULATED, reason="2049 rows: real device only")
@pytest.mark.parametrize("n", [2048, 2049])
def test_etree_budget(n):
    """LDL_BUDGET = 2048 rows per launch: row 2048 climbs from node 3 through links that the first launch made"""
    budget = 2048
    longs = [(n - 1, 3)] if n > budget else []
    m, ref, b, want = _ref("budget%d" % n, lambda: chain_matrix(n, longs, 2048 + n), None)
    assert ref[0][:n - 1] == list(range(1, n))              # the chain: every climb passes all the nodes before it
    sym, _, _ = _device_check(m, ref, b, want)
    assert sym.stats["etree_launches"] == (n + budget - 1) // budget
    assert sym.stats["readbacks"] == 2


# ---- 3. update and repeated factors past one row per wave -------------------------------------------------------------------------

def test_update_and_repeats():
    from sprs_amd.device import DeviceVec
    waves, n, make = _seam_case()
    assert n > 2 * waves
    perm = _seam_perms(n)["reversal"]
    m, ref, b, want = _ref("seam", make, perm)
    sym, num, a = _device_check(m, ref, b, want, perm)
    want_l, want_d = num.l().to_host()[3], num.d().to_host()
    for _ in range(5):                                       # repeated factors are bit-identical
        again = sym.factor(a)
        assert _same_bits(again.l().to_host()[3], want_l) and _same_bits(again.d().to_host(), want_d)
    m2, ref2, _, want2 = _ref("seam-rescaled", lambda: rescaled(m, 4101), perm)
    assert not _same_bits(ref2[4], ref[4]) and not _same_bits(want2, want)
    a2 = _mat(m2)
    num.update(a2)
    _same_factors(sym, num, ref2)
    fresh = sym.factor(a2)
    assert _same_bits(fresh.l().to_host()[3], num.l().to_host()[3]) and _same_bits(fresh.d().to_host(), num.d().to_host())
    assert _same_bits(num.solve(DeviceVec.from_host(b)).to_host(), want2)      # solve after update uses the new values


# ---- 4. two zero pivots in different draws -----------------------------------------------------------------------------------------

def test_two_zero_pivots():
    from sprs_amd import LdlSymbolic, SprsHipError, _ffi
    waves, n, _ = _seam_case()
    first, second = waves + 7, 2 * waves + 1
    assert n > 2 * waves and first // waves < second // waves < n   # rows are drawn in ascending order, WAVES at a time
    ones = {first - 1, first, second - 1, second}
    cuts = {first - 2, first, second - 2, second}            # no link into or out of the two 2 x 2 blocks
    longs = [(r, c) for r, c in seam_longs(n, waves) if r not in ones and c not in ones]
    m = chain_matrix(n, longs, 4102, cuts, ones)
    with pytest.raises(R.Singular) as want:
        R.factor(*m)
    assert want.value.index == first
    parents, _, colptr = R.symbolic(m[0], m[1], m[2])
    _, _, d, singular = R.numeric_closed(*m, None, colptr, parents, stop_at_singular=False)
    assert singular == first and [k for k in range(n) if d[k] == 0.0] == [first, second]
    a = _mat(m)
    sym = LdlSymbolic.new(a)
    assert sym.parents() == parents and sym.colptr().tolist() == colptr
    with pytest.raises(SprsHipError) as e:
        sym.factor(a)
    assert e.value.status == _ffi.SINGULAR_MATRIX and e.value.index == first and e.value.reason == "numeric"
    assert str(want.value) in str(e.value)


# ---- 5. special values ---------------------------------------------------------------------------------------------------------------

def _set_pair(m, r, c, v):
    n, ip, ix, dt = m
    for a, b in ((r, c), (c, r)):
        (p,) = [p for p in range(int(ip[a]), int(ip[a + 1])) if int(ix[p]) == b]
        dt[p] = v


def _nan_aware_same(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    ok = ~np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)) and _same_bits(got[ok], want[ok])


def test_special_values():
    """four independent chains, one stored special value each: +inf, -0.0, a NaN, and the NaN whose bits are all ones (what
    memset 0xFF leaves, the factor's "pending" tag).  Each sits below the diagonal of a chain, so it reaches l_data in its own row
    and d from there on; a long-range entry per chain carries it into a longer row"""
    from sprs_amd import LdlSymbolic
    from sprs_amd.device import DeviceVec
    n = 70
    cuts = {19, 39, 54}
    longs = [(15, 2), (35, 22), (52, 42), (68, 57)]
    m = chain_matrix(n, longs, 70, cuts)
    _set_pair(m, 5, 4, np.inf)
    _set_pair(m, 25, 24, -0.0)
    _set_pair(m, 45, 44, np.nan)
    _set_pair(m, 60, 59, ALL_ONES)
    assert int((R.bits(m[3]) == np.uint64(2**64 - 1)).sum()) == 2
    parents, _, colptr = R.symbolic(m[0], m[1], m[2])
    l_indices, l_data, d, singular = R.numeric_closed(*m, None, colptr, parents, stop_at_singular=False)
    assert singular is None
    l_data, d = np.array(l_data), np.array(d)
    assert np.isinf(l_data).any() and np.isinf(d).any()      # the special values reach both factors
    assert np.isnan(l_data[colptr[40]:]).sum() >= 2 and np.isnan(d[40:55]).any() and np.isnan(d[55:]).any()
    assert l_data[colptr[24]] == 0.0 and not np.signbit(l_data[colptr[24]])   # L[25, 24] = (0.0 + -0.0) / d[24]
    assert not np.isnan(d[20:40]).any()
    a = _mat(m)
    sym = LdlSymbolic.new_perm(a, None, False)               # (NaN != NaN: the symmetry check would refuse the matrix)
    assert sym.parents() == parents and sym.colptr().tolist() == colptr
    num = sym.factor(a)
    _, ip, ix, dt = num.l().to_host()
    assert ip.tolist() == colptr and ix.tolist() == l_indices
    assert _nan_aware_same(dt, l_data)
    assert _nan_aware_same(num.d().to_host(), d)
    b = _rhs(n, 71)
    with np.errstate(all="ignore"):
        want, _ = R.solve(n, colptr, l_indices, l_data.tolist(), d.tolist(), None, b)
    assert np.isnan(want).any() and not np.isnan(want).all()
    assert _nan_aware_same(num.solve(DeviceVec.from_host(b)).to_host(), want)


def test_negative_zero_pivot_is_singular():
    """a stored -0.0 on a diagonal nothing is subtracted from: the pivot is 0.0 + (-0.0) == 0.0, singular at that index"""
    from sprs_amd import LdlNumeric, SprsHipError, _ffi
    n = 6
    m = chain_matrix(n, [(5, 1)], 6, cuts={2, 3})
    (p,) = [p for p in range(int(m[1][3]), int(m[1][4])) if int(m[2][p]) == 3]
    assert int(m[1][4]) - int(m[1][3]) == 1                  # row 3 stores its diagonal only
    m[3][p] = -0.0
    with pytest.raises(R.Singular) as want:
        R.factor(*m)
    assert want.value.index == 3
    with pytest.raises(SprsHipError) as e:
        LdlNumeric.new(_mat(m))
    assert e.value.status == _ffi.SINGULAR_MATRIX and e.value.index == 3 and e.value.reason == "numeric"
    assert str(want.value) in str(e.value)


# ---- 6. past 256 x CUs rows: the clamp of the flag words and the solves' second chunk ------------------------------------------

@pytest.mark.skipif(EMULATED, reason="65 665 rows on an MI355X: real device only")
def test_past_the_grid():
    from sprs_amd import ldl_lsolve, ldl_ltsolve
    from sprs_amd.device import DeviceVec
    cus = _cus()
    n = max(256 * cus, 2**24 // cus) + 129
    assert n > 256 * cus, "one chunk of 64 rows per wave covers the system: the solves draw nothing twice"
    assert n * 32 * (2 * cus) > 2**30, "2 x CUs workgroups of flag words fit into 1 GiB: the clamp does not bind"
    m, ref, b, want = _ref("blocks", lambda: block_matrix(n, 65), None)
    _, colptr, l_indices, l_data, _ = ref
    assert colptr[n] <= 64 * n
    _, num, _ = _device_check(m, ref, b, want, None, CSR, np.uint32, np.uint64)
    l = num.l()
    x = DeviceVec.from_host(b)
    ldl_lsolve(l, x)
    assert _same_bits(x.to_host(), R.ldl_lsolve(n, colptr, l_indices, l_data, [float(v) for v in b]))
    x = DeviceVec.from_host(b)
    ldl_ltsolve(l, x)
    assert _same_bits(x.to_host(), R.ldl_ltsolve(n, colptr, l_indices, l_data, [float(v) for v in b]))
