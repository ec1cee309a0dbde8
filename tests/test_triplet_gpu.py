"""GPU parity of the triplet -> CSR / CSC assembly (sprs_amd/triplet.py, twin of TriMatBase::to_csr /
to_csc, triplet.rs:262-276 -> triplet_iter.rs:127-224) against the oracle's restatement: structure
bit-exact; values bit-exact too, because both fold duplicates in triplet order."""
import os

import numpy as np
import pytest

from helpers import fresh_blocks

pytestmark = pytest.mark.gpu
EMULATED = bool(os.environ.get("SPRS_HIP_LIBRARY"))   # the kernel emulator of tests/emu (tests/test_convert_emu_cpu.py)


@pytest.fixture(scope="module")
def hip():
    import sprs_amd
    if sprs_amd.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X (no CPU fallback exists)")
    return sprs_amd


def random_triplets(rows, cols, n, seed, hot=0.2):
    rng = np.random.default_rng(seed)
    r = rng.integers(0, rows, n)
    c = rng.integers(0, cols, n)
    m = rng.random(n) < hot                                   # a few cells collect many duplicates
    r[m] = rng.integers(0, min(3, rows), m.sum())
    c[m] = rng.integers(0, min(3, cols), m.sum())
    v = rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)  # order of the additions is visible in the bits
    return r, c, v


@pytest.mark.parametrize("idx", [np.uint64, np.uint32])
@pytest.mark.parametrize("storage", ["CSR", "CSC"])
def test_assembly_matches_oracle(hip, storage, idx):
    from oracle import oracle
    from sprs_amd.triplet import TriMat
    rows, cols, n = 700, 450, 60000
    r, c, v = random_triplets(rows, cols, n, seed=3)
    t = TriMat((rows, cols), r, c, v)
    m = t.to_csr(idx) if storage == "CSR" else t.to_csc(idx)
    shape, ip, ix, dt = m.to_host()
    rip, rix, rdt = oracle.triplets_to_cs((rows, cols), r, c, v, storage=storage, idx_dtype=idx)
    assert shape == (rows, cols) and (m.is_csr() if storage == "CSR" else m.is_csc())
    assert ix.dtype == np.dtype(idx)
    assert np.array_equal(ip, rip) and np.array_equal(ix, rix)
    assert np.array_equal(dt, rdt)
    assert int(rip[-1]) < n                                   # duplicates were folded


def test_zeros_cancellation_empty_and_big_rows(hip):
    from oracle import oracle
    from sprs_amd.triplet import TriMat
    # explicit zero, a sum that cancels (stays stored), an empty row, an empty matrix
    t = TriMat((4, 4), [2, 0, 2, 0, 2, 1], [1, 3, 1, 0, 1, 2], [1e16, 5.0, 1.0, 0.0, -1e16, 7.0])
    shape, ip, ix, dt = t.to_csr().to_host()
    rip, rix, rdt = oracle.triplets_to_cs((4, 4), t.row_inds, t.col_inds, t.data)
    assert np.array_equal(ip, rip) and np.array_equal(ix, rix) and np.array_equal(dt, rdt)
    assert dt.tolist() == [0.0, 5.0, 7.0, (1e16 + 1.0) + -1e16]
    e = TriMat((3, 2))
    assert e.to_csr().to_host()[1].tolist() == [0, 0, 0, 0] and e.to_csc().to_host()[1].tolist() == [0, 0, 0]
    # one row collecting 5000 triplets over 40 columns (large-row SpGEMM path of the selector product)
    rng = np.random.default_rng(1)
    n = 5000
    r = np.full(n, 7)
    c = rng.integers(0, 40, n)
    v = rng.standard_normal(n)
    t = TriMat((9, 40), r, c, v)
    shape, ip, ix, dt = t.to_csr().to_host()
    rip, rix, rdt = oracle.triplets_to_cs((9, 40), r, c, v)
    assert np.array_equal(ip, rip) and np.array_equal(ix, rix) and np.array_equal(dt, rdt)


def test_matrix_market_to_device_and_multiply(hip):
    """read -> assemble on the device -> SpMV, against the dense matrix scipy reads from the same text"""
    import io
    import scipy.io
    from sprs_amd.device import DeviceVec
    from sprs_amd.io import read_matrix_market, write_matrix_market
    from sprs_amd.triplet import TriMat
    r, c, v = random_triplets(300, 300, 8000, seed=9, hot=0.05)
    buf = io.StringIO()
    write_matrix_market(buf, TriMat((300, 300), r, c, v))
    text = buf.getvalue()
    a = read_matrix_market(io.StringIO(text)).to_csr()
    dense = scipy.io.mmread(io.BytesIO(text.encode())).toarray()
    x = np.random.default_rng(2).standard_normal(300)
    y = (a * DeviceVec.from_host(x)).to_host()
    assert np.allclose(y, dense @ x, rtol=1e-10, atol=1e-8)
    # and back out through the writer: same matrix
    out = io.StringIO()
    write_matrix_market(out, a)
    assert np.allclose(scipy.io.mmread(io.BytesIO(out.getvalue().encode())).toarray(), dense, rtol=1e-13, atol=1e-13)


def test_reference_golden_cases(hip, golden):
    """the reference's own triplet tests (triplet.rs:343-646, tests/golden/sprs_fixtures.json): to_csc must give the CSC
    it asserts, to_csr that matrix converted (`expected.to_csr()`), for 8- and 4-byte indices"""
    from oracle import oracle
    from sprs_amd.triplet import TriMat
    for c in golden["triplet_cases"]:
        rows, cols = c["shape"]
        exp = c["csc"]
        eip, eix, edt = oracle.convert_storage(cols, rows, np.array(exp["indptr"], dtype=np.uint64),
                                               np.array(exp["indices"], dtype=np.uint64), np.array(exp["data"]))
        for idx in (np.uint64, np.uint32):
            t = TriMat((rows, cols), c["rows"], c["cols"], c["data"])
            shape, ip, ix, dt = t.to_csc(idx).to_host()
            assert shape == (rows, cols)
            assert ip.tolist() == exp["indptr"] and ix.tolist() == exp["indices"] and dt.tolist() == exp["data"], c["name"]
            shape, ip, ix, dt = t.to_csr(idx).to_host()
            assert ip.tolist() == eip.tolist() and ix.tolist() == eix.tolist() and dt.tolist() == edt.tolist(), c["name"]


@pytest.mark.parametrize("storage", ["CSR", "CSC"])
def test_sort_route_equals_selector_product(hip, storage):
    """the radix-sort kernel route (sprs_hip_triplets_to_cs) and the selector-product route (to_other_storage +
    mul_csr_csr) fold duplicates in the same (triplet) order: identical bits; 2e5 triplets with heavy duplication,
    indices that need more than one radix pass in both fields"""
    from sprs_amd.triplet import TriMat
    rows, cols, n = 70000, 300, 40000 if EMULATED else 200000
    r, c, v = random_triplets(rows, cols, n, seed=11, hot=0.3)
    t = TriMat((rows, cols), r, c, v)
    a = (t.to_csr() if storage == "CSR" else t.to_csc()).to_host()
    b = (t.to_csr(method="product") if storage == "CSR" else t.to_csc(method="product")).to_host()
    assert a[0] == b[0]
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x, y)


def test_out_of_bounds_and_widths(hip):
    import ctypes as C
    from sprs_amd import _ffi
    from sprs_amd.device import DeviceVec
    r = DeviceVec.from_host(np.array([0, 5], dtype=np.uint64).view(np.float64))
    c = DeviceVec.from_host(np.array([1, 1], dtype=np.uint64).view(np.float64))
    v = DeviceVec.from_host(np.array([1.0, 2.0]))
    h = C.c_void_p()
    st = _ffi.lib.sprs_hip_triplets_to_cs(4, 4, 2, C.c_void_p(r.ptr), C.c_void_p(c.ptr), 8, C.c_void_p(v.ptr), 0, 8, 8, C.byref(h))
    assert st == _ffi.INVALID_ARG and b"out of bounds" in _ffi.lib.sprs_hip_last_error()
    st = _ffi.lib.sprs_hip_triplets_to_cs(4, 4, 2, C.c_void_p(r.ptr), C.c_void_p(c.ptr), 2, C.c_void_p(v.ptr), 0, 8, 8, C.byref(h))
    assert st == _ffi.INVALID_ARG


# ---- seams of the radix sort, the group scan and the fold: bit-exact against the oracle ----------------------------

def check_assembly(shape, r, c, v, storage, idx=np.uint64):
    from oracle import oracle
    from sprs_amd.triplet import TriMat
    t = TriMat(shape, r, c, v)
    fresh_blocks()
    m = t.to_csr(idx) if storage == "CSR" else t.to_csc(idx)
    s2, ip, ix, dt = m.to_host()
    rip, rix, rdt = oracle.triplets_to_cs(shape, r, c, v, storage=storage, idx_dtype=idx)
    assert tuple(s2) == tuple(shape) and (m.is_csr() if storage == "CSR" else m.is_csc())
    assert ip.dtype == np.uint64 and ix.dtype == np.dtype(idx) and ip.size == (shape[0] if storage == "CSR" else shape[1]) + 1
    assert np.array_equal(ip, rip)
    assert np.array_equal(ix, rix)
    assert np.array_equal(dt.view(np.uint64), rdt.view(np.uint64))
    return ip, ix, dt


@pytest.mark.parametrize("storage", ["CSR", "CSC"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4095, 4096, 4097, 16383, 16384, 16385])
def test_sort_chunk_and_wave_seams(hip, n, storage):
    """one below, on and one above a 64-lane step, a 4096-element wave chunk and a 4-wave workgroup of the radix sort; 1073
    cells for up to 16385 triplets, so the fold order of every cell shows in the value bits"""
    r, c, v = random_triplets(37, 29, n, seed=100 + n)
    ip, _, _ = check_assembly((37, 29), r, c, v, storage)
    assert int(ip[-1]) == np.unique(r * 29 + c).size


@pytest.mark.parametrize("storage", ["CSR", "CSC"])
@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (300, 1), (2, 2), (255, 256), (256, 257), (257, 65536), (65537, 3)])
def test_sort_key_field_widths(hip, shape, storage):
    """key fields of 1, 8, 9, 16 and 17 bits: bits_for at and around the powers of two, full passes and a partial last one"""
    r, c, v = random_triplets(shape[0], shape[1], 5000, seed=shape[0] + 7 * shape[1])
    check_assembly(shape, r, c, v, storage)


def test_sort_32_bit_inner_field(hip):
    """rows = 2^32 - 1 as CSC: the inner field takes all 32 low key bits (four full passes); the top row and row 0 are used"""
    rows, cols, n = (1 << 32) - 1, 4, 3000
    rng = np.random.default_rng(17)
    r = rng.integers(0, rows, n)
    r[rng.permutation(n)[:100]] = np.repeat([rows - 1, 0], 50)
    c = rng.integers(0, cols, n)
    v = rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)
    _, ix, _ = check_assembly((rows, cols), r, c, v, "CSC")
    assert int(ix.max()) == rows - 1 and int(ix.min()) == 0
    from sprs_amd.triplet import TriMat
    with pytest.raises(OverflowError, match="Index type is not large enough"):     # u32 cannot hold 2^32 - 1 rows (SpIndex)
        TriMat((rows, cols), r, c, v).to_csc(np.uint32)


@pytest.mark.parametrize("storage", ["CSR", "CSC"])
@pytest.mark.parametrize("case", ["one_cell", "no_duplicates", "first_row", "last_row"])
def test_grouping_extremes(hip, case, storage):
    rng = np.random.default_rng(23)
    rows, cols = 97, 61
    if case == "one_cell":                  # one group of 9000 in the last cell: its thread writes every indptr entry
        n = 9000
        r, c = np.full(n, rows - 1), np.full(n, cols - 1)
    elif case == "no_duplicates":           # every triplet heads its own group
        cells = rng.permutation(rows * cols)[:5000]
        n, r, c = cells.size, cells // cols, cells % cols
    else:                                   # empty outer slices behind (first row) or before (last row) the only used one
        n = 5000
        r, c = np.full(n, 0 if case == "first_row" else rows - 1), rng.integers(0, cols, n)
    v = rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)
    ip, _, _ = check_assembly((rows, cols), r, c, v, storage)
    assert int(ip[-1]) == {"one_cell": 1, "no_duplicates": n}.get(case, np.unique(c).size)


@pytest.mark.parametrize("storage", ["CSR", "CSC"])
@pytest.mark.parametrize("outer", [255, 256, 257, 512])
def test_empty_trimat_indptr_seams(hip, outer, storage):
    """outer + 1 indptr zeros on both sides of the 256-thread grid of the kernel that writes them"""
    ip, ix, dt = check_assembly((outer, 3) if storage == "CSR" else (3, outer), [], [], [], storage)
    assert ip.tolist() == [0] * (outer + 1) and ix.size == 0 and dt.size == 0


@pytest.mark.parametrize("storage", ["CSR", "CSC"])
@pytest.mark.parametrize("widths", [(4, 4, 4), (4, 8, 4), (8, 4, 4), (4, 8, 8)])
def test_abi_index_widths(hip, widths, storage):
    """sprs_hip_triplets_to_cs with 4-byte input indices, 4-byte output indices and a 4-byte indptr (the Python wrapper
    passes 8, ib, 8 only); every device buffer is exactly as long as its array"""
    import ctypes as C
    from oracle import oracle
    from sprs_amd import _ffi
    from sprs_amd.device import DeviceCsMat
    in_b, idx_b, ptr_b = widths
    dts = {4: np.uint32, 8: np.uint64}
    rows, cols, n = 700, 450, 20000
    r, c, v = random_triplets(rows, cols, n, seed=31)
    bufs = []

    def up(arr):
        arr = np.ascontiguousarray(arr)
        p = C.c_void_p()
        _ffi.check(_ffi.lib.sprs_hip_malloc(C.byref(p), arr.nbytes))
        bufs.append(p)
        _ffi.check(_ffi.lib.sprs_hip_memcpy_h2d(p, C.c_void_p(arr.ctypes.data), arr.nbytes))
        return p

    try:
        pr, pc, pv = up(r.astype(dts[in_b])), up(c.astype(dts[in_b])), up(v)
        h = C.c_void_p()
        fresh_blocks()
        _ffi.check(_ffi.lib.sprs_hip_triplets_to_cs(rows, cols, n, pr, pc, in_b, pv, _ffi.CSR if storage == "CSR" else _ffi.CSC,
                                                    idx_b, ptr_b, C.byref(h)))
        m = DeviceCsMat(h.value)
    finally:
        for p in bufs:
            _ffi.lib.sprs_hip_free(p)
    shape, ip, ix, dt = m.to_host()
    rip, rix, rdt = oracle.triplets_to_cs((rows, cols), r, c, v, storage=storage, idx_dtype=dts[idx_b])
    assert tuple(shape) == (rows, cols) and (m.is_csr() if storage == "CSR" else m.is_csc())
    assert m.index_bytes() == idx_b and m.indptr_bytes() == ptr_b
    assert ip.dtype == np.dtype(dts[ptr_b]) and ix.dtype == np.dtype(dts[idx_b])
    assert np.array_equal(ip, rip.astype(dts[ptr_b])) and int(rip[-1]) < 1 << 32
    assert np.array_equal(ix, rix)
    assert np.array_equal(dt.view(np.uint64), rdt.view(np.uint64))


@pytest.mark.skipif(EMULATED, reason="2^21 triplets: real device only")
def test_two_million_triplets(hip):
    """n = 2^21 + 4097: the scan over the group heads passes 1024 block sums (its third level), and the sort's histogram scan
    runs over 256 * 513 counters"""
    n = (1 << 21) + 4097
    r, c, v = random_triplets(3000, 2500, n, seed=37)
    ip, _, _ = check_assembly((3000, 2500), r, c, v, "CSR")
    assert int(ip[-1]) < n
