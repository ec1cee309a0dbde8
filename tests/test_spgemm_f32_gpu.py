"""The f32 SpGEMM (DeviceCsMatF32 * DeviceCsMatF32, smmp on f32 operands) against the f32 restatement of smmp::numeric
(tests/spgemm_f32_ref.py): indptr and indices equal the CPU oracle's, values equal the reference's f32 chain BIT FOR BIT —
every product rounded to f32, added one at a time from +0.0f in ascending position of k.  An f64 product rounded at the end is
not that chain (tests/test_spgemm_f32_cpu.py shows the inputs tell them apart), so bit-equality here is a test of the order of
the additions in every kernel family: lane groups, hash tables, wave per row, workgroup.

The operands are those of tests/test_spgemm_gpu.py cast to f32 (no product of theirs overflows in f32: the reference stays
finite, asserted where they are used, so no magnitude was rescaled).  The file also runs under the kernel emulator
(tests/test_spgemm_f32_emu_cpu.py); the determinism case is smaller there."""
import os

import numpy as np
import pytest

from conftest import IDX_COMBOS, as_csr
from spgemm_f32_ref import as_f32, as_f64, gamma_bound, mul_csr_csr_f32, product_counts_and_magnitudes, same_bits
from test_spgemm_gpu import _LAUNCH_VARIANTS, _dense_output_case, _order_stress_cases, _row_class_operands, _row_classes

pytestmark = pytest.mark.gpu
EMULATED = bool(os.environ.get("SPRS_HIP_LIBRARY"))     # the kernel emulator of tests/emu


@pytest.fixture(scope="module")
def hip():
    import sprs_amd
    if sprs_amd.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X (no CPU fallback exists)")
    return sprs_amd


class options:
    """set options for a block and put back what they were"""

    def __init__(self, hip, **opts):
        self.hip, self.opts = hip, opts

    def __enter__(self):
        self.was = {k: self.hip.get_option(k) for k in self.opts}
        for k, v in self.opts.items():
            self.hip.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.was.items():
            self.hip.set_option(k, v)


def f32_pair(a, b):
    from sprs_amd.device import DeviceCsMatF32
    return DeviceCsMatF32.from_host(*a), DeviceCsMatF32.from_host(*b)


def gpu_mul(a, b):
    from sprs_amd import smmp
    from sprs_amd.device import DeviceCsMatF32
    da, db = f32_pair(a, b)
    c = smmp.mul_csr_csr(da, db)
    assert type(c) is DeviceCsMatF32 and c.is_csr()
    return c.to_host()


def check_bits(got, ref, what=""):
    assert got[0] == ref[0], what
    assert got[1].dtype == ref[1].dtype and got[2].dtype == ref[2].dtype, what          # same I / Iptr as the operands
    assert np.array_equal(got[1], ref[1]), "indptr differs " + what
    assert np.array_equal(got[2], ref[2]), "indices differ " + what
    assert got[3].dtype == np.float32
    assert same_bits(got[3], ref[3]), "value bits differ %s: %d of %d" % (
        what, int(np.sum(got[3].view(np.uint32) != ref[3].view(np.uint32))), ref[3].size)


# ---- failing without the feature: the product exists and is exact on the golden cases ---------------------------------------
@pytest.mark.parametrize("idx,ptr", IDX_COMBOS)
def test_golden_products_exact(hip, golden, idx, ptr):
    from sprs_amd.device import DeviceCsMatF32
    a, b = as_f32(as_csr(golden["mat1"], idx, ptr)), as_f32(as_csr(golden["mat2"], idx, ptr))
    for rhs, key in ((a, "mat1_self_matprod"), (b, "mat1_matprod_mat2")):
        exp = as_csr(golden[key], idx, ptr)
        got = gpu_mul(a, rhs)                                            # smmp.mul_csr_csr
        assert got[0] == exp[0] and np.array_equal(got[1], exp[1]) and np.array_equal(got[2], exp[2])
        assert got[3].dtype == np.float32 and np.array_equal(got[3].astype(np.float64), exp[3])
        da, db = f32_pair(a, rhs)
        for c in (da * db, da @ db):                                     # the operators
            assert type(c) is DeviceCsMatF32
            assert np.array_equal(c.to_host()[3].astype(np.float64), exp[3]) and np.array_equal(c.to_host()[2], exp[2])


# ---- the routing thresholds --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx,ptr", IDX_COMBOS)
def test_row_class_boundaries(hip, idx, ptr):
    """rows of 64 / 65 and 512 / 513 products, 64 / 65 k's, empty rows of B among the k's, columns on window and bucket edges,
    under the four (spgemm_mid, spgemm_heavy) settings of the f64 test: every row class on both sides of its threshold"""
    A, B, ub, _ = _row_class_operands(idx, ptr)
    assert 64 in ub and 65 in ub and 512 in ub and 513 in ub
    a, b = as_f32(A), as_f32(B)
    ref = mul_csr_csr_f32(a, b)
    assert np.all(np.isfinite(ref[3]))
    for mid, heavy in ((65536, 131072), (max(ub[3] - 1, 513), 131072), (ub[3], 1024), (0, 2048)):
        with options(hip, spgemm_mid=mid, spgemm_heavy=heavy):
            check_bits(gpu_mul(a, b), ref, "(mid %d, heavy %d)" % (mid, heavy))


# ---- lane groups -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx,ptr", IDX_COMBOS)
def test_micro_lane_groups(hip, idx, ptr):
    """rows of <= 16 / 32 / 64 products and k's on lane groups, and on the hash kernel (spgemm_micro = 2): lengths 1, 2, 3, the
    class edges 16 / 17, 32 / 33, 64 / 65, k's outnumbering products, long runs of one column — and rows of B that START AT ODD
    entry positions (B's rows of 1 and 3 entries put every later row on an odd position: an 8-byte record loaded in pairs
    would straddle)"""
    rng = np.random.default_rng(91)
    cols = 300
    b_lens = [1, 3, 1, 2, 5, 4, 7, 8, 1, 16, 15, 17, 3, 32, 31, 33, 1, 64, 63, 65, 0, 0, 12, 12, 12, 12, 9, 1, 1, 1]
    b_rows = [sorted(rng.choice(cols, size=n, replace=False).tolist()) if n != 12 else sorted(rng.choice(20, size=12, replace=False).tolist())
              for n in b_lens]
    b_ip = np.concatenate([[0], np.cumsum(b_lens)])
    assert sum(1 for s, n in zip(b_ip[:-1], b_lens) if n and s % 2) >= 8           # rows that start at odd positions
    b_ix = np.array([c for r in b_rows for c in r], dtype=np.int64)
    b_dt = (rng.standard_normal(b_ix.size) * 10.0 ** rng.integers(-12, 13, size=b_ix.size)).astype(np.float32)
    B = ((len(b_lens), cols), b_ip.astype(ptr), b_ix.astype(idx), b_dt)
    a_rows = [[0], [2], [3], [1], [0, 2], [0, 1, 2], [3, 12],              # 1, 1, 2, 3 products; 2, 5, 5
              [9], [11], [13], [15], [17], [19], [10], [14], [18],         # single k's: 16, 17, 32, 33, 64, 65, 15, 31, 63 products
              [4, 5, 6], [4, 5, 6, 8], [6, 7, 9], [6, 7, 9, 16],           # 16 / 17 and 31 / 32 products from several k's
              [20, 21, 22],                                                # empty rows of B among the k's
              [22, 23, 24, 25],                                            # 48 products on 20 columns: long chains per column
              [22, 23, 24, 25, 26, 27],                                    # 58 products
              [0, 2, 8, 16, 27, 28, 29] + [20, 21],                        # nine k's of one entry or none
              list(range(0, 9)),                                           # 32 products, 9 k's
              [], [27]]
    a_rows = [sorted(r) for r in a_rows]
    a_ip = np.concatenate([[0], np.cumsum([len(r) for r in a_rows])])
    a_ix = np.array([k for r in a_rows for k in r], dtype=np.int64)
    a_dt = (rng.standard_normal(a_ix.size) * 10.0 ** rng.integers(-12, 13, size=a_ix.size)).astype(np.float32)
    A = ((len(a_rows), len(b_lens)), a_ip.astype(ptr), a_ix.astype(idx), a_dt)
    ub = [sum(b_lens[k] for k in r) for r in a_rows]
    assert {1, 2, 3, 16, 17, 32, 33, 64, 65} <= set(ub)
    classes = set(_row_classes(ub, [len(r) for r in a_rows], 65536, True))
    assert {"micro16", "micro32", "micro64", "small"} <= classes
    ref = mul_csr_csr_f32(A, B)
    assert np.all(np.isfinite(ref[3]))
    for micro in (0, 2):
        with options(hip, spgemm_micro=micro):
            check_bits(gpu_mul(A, B), ref, "(spgemm_micro %d)" % micro)


# ---- the order of the additions ----------------------------------------------------------------------------------------------
_STRESS = []


def _stress_cases_f32():
    """the seven order-stress cases cast to f32 with their f32 references and the f64 product of the same f32 operands"""
    if not _STRESS:
        from oracle import oracle
        for a, b in _order_stress_cases():
            a32, b32 = as_f32(a), as_f32(b)
            ref64 = oracle.mul_csr_csr(*as_f64(a32), *as_f64(b32), threads=1)
            _STRESS.append((a32, b32, mul_csr_csr_f32(a32, b32, structure=ref64), ref64))
    return _STRESS


@pytest.mark.parametrize("lane_order,lds_atomic", [(0, 1), (2, 1), (2, 0)])
def test_order_of_additions_stress(hip, lane_order, lds_atomic):
    """one LDS add per wave instruction (where the device passed the f32 probe) / one per k-run / read-add-write per k-run: the same
    bits, the reference's, on inputs where any reordering shows"""
    for n, (a, b, ref, ref64) in enumerate(_stress_cases_f32()):
        assert np.all(np.isfinite(ref[3]))                               # no overflow: magnitudes as in the f64 test
        assert not same_bits(ref[3], ref64[3].astype(np.float32))        # the input discriminates
        with options(hip, spgemm_lane_order=lane_order, spgemm_lds_atomic=lds_atomic):
            check_bits(gpu_mul(a, b), ref, "(case %d)" % n)


@pytest.mark.parametrize("winlog", [16, 17, 18, 19])
def test_window_widths_and_passes(hip, winlog):
    """every LDS layout of the workgroup kernel with more than ACC_CAP outputs in a window (several passes), ~600 k's per row
    (several staged groups), heavy rows cut into narrow windows; with the bucket table and with binary searches"""
    A, B, ref64 = _dense_output_case()
    a, b = as_f32(A), as_f32(B)
    if not _DENSE_REF:                                                   # computed once for the four window widths
        _DENSE_REF.append(mul_csr_csr_f32(a, b, structure=ref64))        # (the structure does not depend on the values)
    ref = _DENSE_REF[0]
    assert np.diff(ref[1].astype(np.int64)).max() > 100_000
    for bucket in (1, 0):
        with options(hip, spgemm_winlog=winlog, spgemm_heavy=4096, spgemm_bucket=bucket):
            check_bits(gpu_mul(a, b), ref, "(winlog %d, bucket %d)" % (winlog, bucket))


_DENSE_REF = []


@pytest.mark.parametrize("idx,ptr", [(np.uint64, np.uint64), (np.uint32, np.uint32)])
def test_launch_variants(hip, idx, ptr):
    """every option that picks an instantiation, a flag word or a stream of the launches, one at a time, on one matrix that
    routes rows to every kernel family; the kept-plan path under the two variants the f64 test runs it for"""
    from sprs_amd import smmp
    A, B, ub, nk = _row_class_operands(idx, ptr)
    a, b = as_f32(A), as_f32(B)
    ref = mul_csr_csr_f32(a, b)
    for opts, kept in _LAUNCH_VARIANTS:
        with options(hip, **opts):
            classes = set(_row_classes(ub, nk, hip.get_option("spgemm_mid"), hip.get_option("spgemm_micro") != 2))
            short = {"tiny"} if opts.get("spgemm_micro") == 2 else {"micro16", "micro32", "micro64"}
            assert classes & short and classes & {"tiny", "small"} and "mid" in classes and "large" in classes, (opts, classes)
            check_bits(gpu_mul(a, b), ref, str(opts))
            if kept:
                da, db = f32_pair(a, b)
                plan = smmp.SpgemmPlan(da, db)
                st = plan.structure()
                plan.numeric(st)
                check_bits(st.to_host(), ref, "kept plan " + str(opts))


# ---- special values ----------------------------------------------------------------------------------------------------------
def test_special_values_by_hand(hip):
    """one row per case, all tiny (lane groups, and the hash kernel under spgemm_micro = 2): a lone product of -0.0 gives +0.0
    (the chain starts at +0.0f); subnormal products; a sum that ends subnormal; a product that overflows in f32 but not in
    f64; inf - inf; NaN operands; stored zeros kept"""
    f = np.float32
    u = lambda *v: np.array(v, dtype=np.uint64)
    # B: row k has the single entry (k, column 0) except rows 8, 9 (two columns)
    b_dt = np.array([0.0, 1e-20, 2.0, -1.5, 1e20, 1e20, -1e20, np.nan, 0.0, 0.0, 1.0, 1.0], dtype=f)
    B = ((10, 2), u(0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12), u(0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1), b_dt)
    a_rows = [([0], [-1.0]),                         # -1 * 0 = -0.0 -> +0.0 + -0.0 = +0.0
              ([1], [1e-20]),                        # 1e-40: a subnormal product
              ([2, 3], [1e-38, 1e-38]),              # 2e-38 - 1.5e-38 = 5e-39: the sum ends subnormal
              ([1, 2], [1e-20, 1e-39]),              # a subnormal product plus the product of a subnormal operand
              ([4], [1e20]),                         # 1e40 -> +inf in f32, finite in f64
              ([5, 6], [1e20, 1e20]),                # inf - inf -> NaN
              ([7], [1.0]),                          # a NaN in B
              ([2], [np.nan]),                       # a NaN in A
              ([8, 9], [5.0, 0.0]),                  # stored zeros: 5 * 0 and 0 * 1 -> zeros kept in the structure
              ([9], [0.0])]
    a_ip = np.concatenate([[0], np.cumsum([len(r[0]) for r in a_rows])]).astype(np.uint64)
    a_ix = np.array([k for r in a_rows for k in r[0]], dtype=np.uint64)
    with np.errstate(over="ignore"):
        a_dt = np.array([v for r in a_rows for v in r[1]], dtype=f)
    A = ((len(a_rows), 10), a_ip, a_ix, a_dt)
    ref = mul_csr_csr_f32(A, B)
    v = ref[3]
    row = lambda i: v[int(ref[1][i]):int(ref[1][i + 1])]
    assert row(0).view(np.uint32)[0] == 0                                # +0.0, not -0.0
    tiny = np.finfo(f).tiny
    assert 0 < row(1)[0] < tiny and 0 < row(2)[0] < tiny and 0 < row(3)[0] < tiny
    assert np.isposinf(row(4)[0]) and np.isnan(row(5)[0]) and np.isnan(row(6)[0]) and np.isnan(row(7)[0])
    assert row(8).size == 2 and not row(8).any() and row(9).size == 2 and not row(9).any()
    for micro in (0, 2):
        with options(hip, spgemm_micro=micro):
            check_bits(gpu_mul(A, B), ref, "(spgemm_micro %d)" % micro)


@pytest.mark.parametrize("scale_a,scale_b,what", [(1e-19, 1e-19, "subnormal"), (1e19, 3e19, "overflow")])
def test_special_values_in_every_kernel_family(hip, scale_a, scale_b, what):
    """the row-class operands scaled so that (subnormal) most products and many sums are f32 subnormals, some flushing to zero by
    rounding, or (overflow) products overflow to +-inf and inf - inf gives NaN — in rows of every class, so that the LDS adds of
    the hash, wave-per-row and workgroup kernels see them, under the three forms of the add"""
    A, B, ub, nk = _row_class_operands(np.uint64, np.uint64)
    with np.errstate(over="ignore"):
        a = (A[0], A[1], A[2], (A[3] * scale_a).astype(np.float32))
        b = (B[0], B[1], B[2], (B[3] * scale_b).astype(np.float32))
    ref = mul_csr_csr_f32(a, b)
    tiny = np.finfo(np.float32).tiny
    if what == "subnormal":
        sub = (np.abs(ref[3]) < tiny) & (ref[3] != 0)
        assert sub.sum() > ref[3].size // 10
    else:
        assert np.isinf(ref[3]).sum() > 100 and np.isnan(ref[3]).sum() > 100 and np.isfinite(ref[3]).sum() > 100
    for lane_order, lds_atomic in ((0, 1), (2, 1), (2, 0)):
        with options(hip, spgemm_lane_order=lane_order, spgemm_lds_atomic=lds_atomic):
            check_bits(gpu_mul(a, b), ref, "(%s, lane_order %d, lds_atomic %d)" % (what, lane_order, lds_atomic))


# ---- kept plan ---------------------------------------------------------------------------------------------------------------
def _rmat(n, per, seed, idx=np.uint64, ptr=np.uint64):
    from sprs_amd import gen
    indptr, indices, data = gen.rmat_csr(n, per, seed=seed)
    return (n, n), indptr.numpy().astype(ptr), indices.numpy().astype(idx), data.numpy().astype(np.float32)


@pytest.mark.parametrize("idx,ptr", IDX_COMBOS)
def test_kept_plan(hip, idx, ptr):
    """structure() = zeros on the oracle's structure; numeric() into it = the reference, twice the same bits; with the values of
    other handles over the same pattern = their reference; a c of another structure is refused"""
    from sprs_amd import smmp
    from sprs_amd.device import DeviceCsMatF32
    n = 1500 if EMULATED else 4000
    a = _rmat(n, 8, 21, idx, ptr)
    ref = mul_csr_csr_f32(a, a)
    da = DeviceCsMatF32.from_host(*a)
    plan = smmp.SpgemmPlan(da, da)
    assert plan.nnz() == ref[3].size
    st = plan.structure()
    assert type(st) is DeviceCsMatF32
    got = st.to_host()
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]) and got[3].dtype == np.float32
    assert not got[3].view(np.uint32).any()                              # 0.0f everywhere, +0.0
    check_bits(plan.product().to_host(), ref, "product()")
    plan.numeric(st)
    first = st.to_host()
    check_bits(first, ref, "numeric()")
    plan.numeric(st)
    assert np.array_equal(st.to_host()[3].view(np.uint32), first[3].view(np.uint32))
    # smmp.symbolic / smmp.numeric without a kept plan
    sym = smmp.symbolic(da, da)
    assert type(sym) is DeviceCsMatF32 and not sym.to_host()[3].any() and np.array_equal(sym.to_host()[2], ref[2])
    check_bits(smmp.numeric(da, da, sym).to_host(), ref, "smmp.numeric")
    # other values on the same pattern
    a2 = (a[0], a[1], a[2], (a[3] * np.float32(3.0) + np.float32(0.25)).astype(np.float32))
    da2 = DeviceCsMatF32.from_host(*a2)
    smmp.SpgemmPlan(da2, da2).numeric(st)
    check_bits(st.to_host(), mul_csr_csr_f32(a2, a2, structure=ref), "other values")
    other = da * DeviceCsMatF32.from_host((n, n), np.arange(n + 1, dtype=ptr), np.arange(n, dtype=idx), np.ones(n, dtype=np.float32))
    with pytest.raises(hip.SprsHipError) as e:
        plan.numeric(other)
    assert e.value.status == hip._ffi.BAD_STRUCTURE


def test_kept_plan_in_place_values_and_both_precisions_torch_tensors(hip):
    """Handles wrapped over torch tensors: after the values of a and b change IN PLACE (and refresh), numeric() gives the new
    reference.  A plan made from f32 handles serves f64 handles wrapped over the SAME indptr / indices tensors and gives the f64
    oracle's values, and the reverse: a plan holds structure only."""
    import torch
    from oracle import oracle
    from sprs_amd import smmp
    from sprs_amd.device import DeviceCsMat, DeviceCsMatF32
    n = 4000
    a = _rmat(n, 8, 33)
    dev = torch.device("cuda:0")
    ip_t = torch.from_numpy(a[1].astype(np.int64)).to(dev)
    ix_t = torch.from_numpy(a[2].astype(np.int64)).to(dev)
    v32 = torch.from_numpy(a[3]).to(dev)
    v64 = torch.from_numpy(a[3].astype(np.float64) * 1.0000001 + 1e-3).to(dev)
    a32 = DeviceCsMatF32.wrap_torch((n, n), ip_t, ix_t, v32)
    a64 = DeviceCsMat.wrap_torch((n, n), ip_t, ix_t, v64)
    ref32 = mul_csr_csr_f32(a, a)
    a64_host = (a[0], a[1], a[2], v64.cpu().numpy())
    ref64 = oracle.mul_csr_csr(*a64_host, *a64_host, threads=1)
    plan32 = smmp.SpgemmPlan(a32, a32)
    c32 = plan32.structure()
    plan32.numeric(c32)
    check_bits(c32.to_host(), ref32, "f32 plan, f32 handles")
    served = plan32.serving(a64, a64)                                    # the f32 plan, f64 handles
    c64 = served.product().to_host()
    assert np.array_equal(c64[1], ref64[1]) and np.array_equal(c64[2], ref64[2])
    assert np.array_equal(c64[3].view(np.uint64), ref64[3].view(np.uint64))
    plan64 = smmp.SpgemmPlan(a64, a64)                                   # the reverse
    check_bits(plan64.serving(a32, a32).product().to_host(), ref32, "f64 plan, f32 handles")
    # new values in place
    v32.mul_(1.5).add_(0.125)
    torch.cuda.synchronize()
    a32.refresh()
    a_new = (a[0], a[1], a[2], v32.cpu().numpy())
    plan32.numeric(c32)
    check_bits(c32.to_host(), mul_csr_csr_f32(a_new, a_new, structure=ref32), "after the in-place change")


# ---- storage dispatch and contracts ------------------------------------------------------------------------------------------
def test_storage_dispatch(hip):
    """`a * b` for (CSR | CSC) x (CSR | CSC): csmat.rs:1895-1949.  The result has the storage of the lhs.  A CSC lhs is computed
    as (b^T a^T)^T: the reference chain of THAT product (C^T = B^T A^T, k ascending in B^T's row) is the expected value."""
    from sprs_amd import _ffi
    from sprs_amd.device import DeviceCsMatF32
    from helpers import ragged_csr
    import scipy.sparse as sp
    rng = np.random.default_rng(8)
    a = as_f32(ragged_csr([int(v) for v in rng.integers(0, 30, size=70)], 90, seed=1, positive=False))
    b = as_f32(ragged_csr([int(v) for v in rng.integers(0, 30, size=90)], 110, seed=2, positive=False))
    u = lambda v: np.asarray(v).astype(np.uint64)

    def other(m):                                                        # (shape, indptr, indices, data) in the other storage order
        s = sp.csr_matrix((m[3], m[2].astype(np.int64), m[1].astype(np.int64)), shape=m[0]).tocsc()
        s.sort_indices()
        return m[0], u(s.indptr), u(s.indices), s.data.astype(np.float32)

    a_csc, b_csc = other(a), other(b)
    ref_csr = mul_csr_csr_f32(a, b)                                      # lhs CSR: A * B by rows
    # lhs CSC: the CSC arrays of B and A are the CSR arrays of B^T and A^T
    t = lambda m: ((m[0][1], m[0][0]), m[1], m[2], m[3])
    ref_csc = mul_csr_csr_f32(t(b_csc), t(a_csc))
    dev = lambda m, st: DeviceCsMatF32.from_host(*m, storage=st)
    for la, lst in ((a, _ffi.CSR), (a_csc, _ffi.CSC)):
        for rb, rst in ((b, _ffi.CSR), (b_csc, _ffi.CSC)):
            c = dev(la, lst) * dev(rb, rst)
            assert type(c) is DeviceCsMatF32 and c.storage() == lst
            got = c.to_host()
            assert got[0] == (70, 110)
            ref = ref_csr if lst == _ffi.CSR else ref_csc
            assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
            assert same_bits(got[3], ref[3]), (lst, rst)


def test_contracts(hip, golden):
    from sprs_amd import SprsHipError, _ffi, smmp
    from sprs_amd.device import DeviceCsMat, DeviceCsMatF32
    m3 = DeviceCsMatF32.from_host(*as_f32(as_csr(golden["mat3"])))       # 5 x 4
    with pytest.raises(SprsHipError, match="Dimension mismatch") as e:
        smmp.mul_csr_csr(m3, m3)
    assert e.value.status == _ffi.DIM_MISMATCH
    with pytest.raises(SprsHipError, match="Dimension mismatch"):
        m3 * m3
    shape, ip, ix, dt = as_f32(as_csr(golden["mat1_csc"]))
    csc = DeviceCsMatF32.from_host(shape, ip, ix, dt, storage=_ffi.CSC)
    sq = DeviceCsMatF32.from_host(*as_f32(as_csr(golden["mat1"])))
    with pytest.raises(SprsHipError, match="Storage mismatch") as e:
        smmp.mul_csr_csr(sq, csc)
    assert e.value.status == _ffi.STORAGE_MISMATCH
    b32 = DeviceCsMatF32.from_host(*as_f32(as_csr(golden["mat1"], np.uint32, np.uint32)))
    for f in (smmp.mul_csr_csr, lambda x, y: x * y, smmp.symbolic):
        with pytest.raises(SprsHipError) as e:                           # operands share I / Iptr (smmp.rs:196-199)
            f(sq, b32)
        assert e.value.status == _ffi.STORAGE_MISMATCH
    # precisions do not mix: TypeError naming the conversion, from every door
    sq64 = DeviceCsMat.from_host(*as_csr(golden["mat1"]))
    for f in (lambda: sq * sq64, lambda: sq64 * sq, lambda: sq @ sq64, lambda: sq64 @ sq, lambda: smmp.mul_csr_csr(sq, sq64),
              lambda: smmp.mul_csr_csr(sq64, sq), lambda: smmp.symbolic(sq64, sq), lambda: smmp.SpgemmPlan(sq, sq64)):
        with pytest.raises(TypeError, match="to_f64|to_f32"):
            f()
    c64 = smmp.symbolic(sq64, sq64)
    with pytest.raises(TypeError, match="to_f64|to_f32"):
        smmp.numeric(sq, sq, c64)                                        # an f64 c for the f32 numeric
    with pytest.raises(TypeError, match="to_f64|to_f32"):
        smmp.SpgemmPlan(sq, sq).numeric(c64)


def test_iptr_overflow_u32(hip):
    """Iptr::from_usize panics when nnz(C) does not fit (smmp.rs:121): 70000 x 1 times 1 x 70000 has 4.9e9 > 2^32 entries"""
    from sprs_amd import SprsHipError, _ffi, smmp
    from sprs_amd.device import DeviceCsMatF32
    n = 70000
    one = np.ones(n, dtype=np.float32)
    a = DeviceCsMatF32.from_host((n, 1), np.arange(n + 1, dtype=np.uint32), np.zeros(n, dtype=np.uint32), one)
    b = DeviceCsMatF32.from_host((1, n), np.array([0, n], dtype=np.uint32), np.arange(n, dtype=np.uint32), one)
    with pytest.raises(SprsHipError, match="Index type is not large enough") as e:
        smmp.mul_csr_csr(a, b)
    assert e.value.status == _ffi.INDEX_OVERFLOW


# ---- unordered adds, determinism ---------------------------------------------------------------------------------------------
def test_unordered_adds(hip):
    """spgemm_ordered = 0: the structure is exact; every value is a sum of the same rounded products in some order, so it lies
    within γ_m Σ|a b| of the exact (f64) value, m = 1 + the entry's product count, u = 2^-24"""
    for a, b, ref, ref64 in _stress_cases_f32()[:4]:                     # the four routes of the workgroup kernel
        counts, mag = product_counts_and_magnitudes(a, b)
        with options(hip, spgemm_ordered=0):
            got = gpu_mul(a, b)
        assert np.array_equal(got[1], ref64[1]) and np.array_equal(got[2], ref64[2])
        assert np.all(np.abs(got[3].astype(np.float64) - ref64[3]) <= gamma_bound(counts, mag))
    assert hip.get_option("spgemm_ordered") == 1


def test_five_products_identical(hip):
    from sprs_amd.device import DeviceCsMatF32
    n = 3000 if EMULATED else 20000
    da = DeviceCsMatF32.from_host(*_rmat(n, 8, 5))
    db = DeviceCsMatF32.from_host(*_rmat(n, 8, 6))
    first = (da * db).to_host()
    assert first[3].size > 8 * n
    for _ in range(4):
        again = (da * db).to_host()
        assert np.array_equal(again[1], first[1]) and np.array_equal(again[2], first[2])
        assert np.array_equal(again[3].view(np.uint32), first[3].view(np.uint32))
