"""Device orderings — cuthill_mckee_custom / reverse_cuthill_mckee with the three start strategies and both directions,
is_symmetric, degrees, max_outer_nnz (sprs/src/sparse/linalg/ordering.rs, symmetric.rs, csmat.rs:1188-1216) — against the
restatement tests/ordering_ref.py: perm, perm_inv and connected_parts are compared for exact equality, no tolerance anywhere.

The small cases also run against the kernel emulator (tests/test_ordering_emu_cpu.py); the large and the torch cases need a real
device."""
import json
import math
import os

import numpy as np
import pytest

import ordering_ref as R
import perm_ref
from conftest import IDX_COMBOS, ROOT, as_csr
from helpers import ragged_csr

pytestmark = pytest.mark.gpu

EMULATED = bool(os.environ.get("SPRS_HIP_LIBRARY"))
large = pytest.mark.skipif(EMULATED, reason="large case: needs a real device")
CSR, CSC = 0, 1
WIDTHS = IDX_COMBOS + [(np.uint16, np.uint16)]
PAIRS = [(s, d) for s in R.STRATEGIES for d in (R.FORWARD, R.REVERSED)]
BUDGET = 16384                                       # steps of the one-workgroup kernel per launch (OD_BUDGET, ordering.hpp)


@pytest.fixture(scope="module", autouse=True)
def _need_device():
    import sprs_amd
    if sprs_amd.device_count() < 1:
        pytest.skip("no HIP device")


@pytest.fixture(autouse=True)
def _default_options():
    import sprs_amd
    yield
    sprs_amd.set_option("ordering_narrow_cap", 1024)
    sprs_amd.set_option("ordering_key_bits", 64)


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(ROOT, "tests", "golden", "ordering_fixtures.json")) as f:
        return json.load(f)


def _mat(m, storage=CSR, idx=np.uint64, ptr=np.uint64):
    from sprs_amd.device import DeviceCsMat
    shape, ip, ix, dt = m
    return DeviceCsMat.from_host(tuple(shape), np.asarray(ip).astype(ptr), np.asarray(ix).astype(idx), np.asarray(dt, dtype=np.float64),
                                 storage=storage)


def _order(a, strategy, direction, cap=None, **kw):
    import sprs_amd
    from sprs_amd import ordering as O
    if cap is not None:
        sprs_amd.set_option("ordering_narrow_cap", cap)
    return O.cuthill_mckee_custom(a, strategy, direction, **kw)


def _same(o, want):
    perm, parts = want
    assert o.perm.vec().tolist() == perm
    assert o.perm.inv_vec().tolist() == R.perm_inv(perm)
    assert o.connected_parts.tolist() == parts
    assert o.dim == len(perm) and o.stats["components"] == len(parts) - 1


def _check_all(m, pairs=PAIRS, caps=(None, 8, 0), storage=CSR, idx=np.uint64, ptr=np.uint64):
    a = _mat(m, storage, idx, ptr)
    for strategy, direction in pairs:
        want = R.cuthill_mckee(m, strategy, direction)
        for cap in caps:
            _same(_order(a, strategy, direction, 1024 if cap is None else cap), want)


# ---- graphs ----------------------------------------------------------------------------------------------------------------------

def eye(n):
    return (n, n), np.arange(n + 1), np.arange(n), np.ones(n)


def grid_laplacian(nx, ny, shuffle_seed=None):
    idx = np.arange(nx * ny).reshape(nx, ny)
    if shuffle_seed is not None:
        idx = np.random.default_rng(shuffle_seed).permutation(nx * ny).reshape(nx, ny)
    edges = [(int(idx[i, j]), int(idx[i + 1, j])) for i in range(nx - 1) for j in range(ny)]
    edges += [(int(idx[i, j]), int(idx[i, j + 1])) for i in range(nx) for j in range(ny - 1)]
    shape, ip, ix, dt = R.from_edges(nx * ny, edges)
    rows = np.repeat(np.arange(nx * ny), np.diff(ip))
    dt = np.where(ix == rows, 4.0, -1.0)
    return shape, ip, ix, dt


def path(n, first=0):
    return [(first + i, first + i + 1) for i in range(n - 1)]


def broom(cap=8):
    """a path of 20, then a vertex with cap + 1 leaves, then a path again"""
    hub = 19
    edges = path(20)
    leaves = list(range(20, 20 + cap + 1))
    edges += [(hub, v) for v in leaves]
    edges += [(leaves[0], leaves[-1] + 1)] + path(10, leaves[-1] + 1)
    return R.from_edges(leaves[-1] + 11, edges)


def star(leaves):
    n = leaves + 1
    # centre = vertex 0: row 0 holds every vertex; row v holds 0 and v
    ip = np.zeros(n + 1, dtype=np.int64)
    ip[1] = n
    ip[2:] = n + 2 * np.arange(1, n)
    ix = np.empty(n + 2 * (n - 1), dtype=np.int64)
    ix[:n] = np.arange(n)
    ix[n::2] = 0
    ix[n + 1::2] = np.arange(1, n)
    return (n, n), ip, ix, np.ones(ix.size)


def complete(n):
    return (n, n), np.arange(n + 1) * n, np.tile(np.arange(n), n), np.ones(n * n)


def two_swap_graph():
    """the George-Liu loop swaps twice here (asserted with the restatement in tests/test_ordering_cpu.py)"""
    return R.from_edges(9, [(1, 0), (2, 1), (3, 1), (4, 2), (5, 4), (6, 2), (7, 3), (8, 5), (4, 0)])


def contender_tie_graph():
    """0 - 1 - 4 and 0 - 2 - 3: the last level of the structure rooted at 0 is [4, 3] (4's owner comes first), both of degree 1:
    the contender is 4, the smaller id 3 would be wrong.  -> (matrix, root, contender, the tie's other vertex)"""
    return R.from_edges(5, [(0, 1), (0, 2), (1, 4), (2, 3)]), 0, 4, 3


# ---- 1. the reference's own tests ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("idx,ptr", WIDTHS)
@pytest.mark.parametrize("storage", [CSR, CSC])
def test_golden(fx, storage, idx, ptr):
    from sprs_amd import ordering as O
    c = fx["unconnected_graph_lap"]
    lap = _mat(as_csr(c["mat"]), storage, idx, ptr)
    o = O.reverse_cuthill_mckee(lap)
    _same(o, (c["reverse_cuthill_mckee"]["perm"], c["reverse_cuthill_mckee"]["connected_parts"]))
    assert o.perm.index_bytes() == np.dtype(idx).itemsize and o.perm.vec().dtype == idx and not o.perm.is_identity_variant()
    e3 = _mat(eye(3), storage, idx, ptr)
    assert O.reverse_cuthill_mckee(e3).perm.vec().tolist() == fx["eye3"]["reversed"]
    assert O.cuthill_mckee_custom(e3, O.start.PseudoPeripheral.new(), O.order.Forward.new()).perm.vec().tolist() == fx["eye3"]["forward"]
    assert O.is_symmetric(_mat(as_csr(fx["is_symmetric_simple"]), storage, idx, ptr))
    assert O.is_symmetric(lap)


# ---- 2. random symmetric patterns, the three caps --------------------------------------------------------------------------------

SIZES = [1, 2, 3, 5, 8, 9, 10, 17, 33, 64, 65, 100, 129, 200, 257, 300]


@pytest.mark.parametrize("n", SIZES)
def test_random_symmetric_patterns(n):
    if EMULATED and n > 70:
        pytest.skip("large case: needs a real device")
    for seed in range(2):
        _check_all(R.random_pattern(n, 77 * n + seed, True, density=None if seed else 1.2))


@pytest.mark.parametrize("idx,ptr", WIDTHS)
@pytest.mark.parametrize("storage", [CSR, CSC])
def test_widths_and_storages(storage, idx, ptr):
    _check_all(R.random_pattern(40, 5, True, density=1.5), storage=storage, idx=idx, ptr=ptr)


# ---- 3. the narrow <-> wide seam -------------------------------------------------------------------------------------------------

def test_seam_grid_grows_past_the_cap_and_shrinks_back():
    side = 12 if EMULATED else 40
    m = grid_laplacian(side, side)
    a = _mat(m)
    for strategy, direction in PAIRS:
        want = R.cuthill_mckee(m, strategy, direction)
        _same(_order(a, strategy, direction, 8), want)
        _same(_order(a, strategy, direction, 1024), want)


def test_seam_broom():
    _check_all(broom(8), caps=(None, 8, 7, 9, 0))


def test_two_pass_sort_route():
    """ordering_key_bits below the key's width: wide levels sort by id first, then stably by (owner, degree)"""
    import sprs_amd
    m = R.random_pattern(60, 3, True, density=2.0)
    a = _mat(m)
    for strategy, direction in PAIRS:
        want = R.cuthill_mckee(m, strategy, direction)
        sprs_amd.set_option("ordering_key_bits", 1)
        _same(_order(a, strategy, direction, 0), want)
        _same(_order(a, strategy, direction, 2), want)
        sprs_amd.set_option("ordering_key_bits", 64)


# ---- 4. ties and sort width ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("leaves", [300, pytest.param(5000, marks=large), pytest.param(70000, marks=large)])
def test_star(leaves):
    """all leaves of equal degree: the order is by id; the centre's row is longer than a tile; 70000 candidates in one level"""
    m = star(leaves)
    pairs = PAIRS if leaves < 70000 else [(R.PSEUDO_PERIPHERAL, R.REVERSED), (R.MINIMUM_DEGREE, R.FORWARD)]
    _check_all(m, pairs=pairs, caps=(None, 8) if leaves > 300 else (None, 8, 0))


def test_complete_graph_65():
    _check_all(complete(65))


# ---- 5. components ---------------------------------------------------------------------------------------------------------------

def test_components_small(fx):
    _check_all(as_csr(fx["unconnected_graph_lap"]["mat"]))
    _check_all(eye(70), caps=(None, 8))
    paths = []
    for c in range(20):
        paths += path(3, 3 * c)
    _check_all(R.from_edges(60, paths, diag=False))
    # an isolated vertex that has only a diagonal entry, between two edges; and one without any entry
    _check_all(R.from_edges(6, [(0, 1), (3, 4)], diag=True))
    m = R.from_edges(6, [(0, 1), (3, 4)], diag=False)
    shape, ip, ix, dt = m
    ix2 = np.insert(ix, ip[2], 2)                    # (2, 2) stored, vertex 5 has an empty row
    ip2 = ip.copy()
    ip2[3:] += 1
    _check_all((shape, ip2, ix2, np.ones(ix2.size)))


@large
def test_components_large():
    _check_all(eye(5000), caps=(None,))
    paths = []
    for c in range(1000):
        paths += path(3, 3 * c)
    _check_all(R.from_edges(3000, paths), caps=(None,))


@large
@pytest.mark.parametrize("kind", ["eye", "path"])
def test_launches_do_not_grow_with_n(kind):
    """One launch of the one-workgroup kernel runs up to BUDGET steps (a level, a start vertex, the end of a search), and every
    launch is followed by one read-back of the state.  eye(n) takes 3 n + 1 steps; a path of n takes at most 3 n + 16 under the
    pseudo-peripheral search (two level structures of n levels and the order's n levels).  Besides them a call makes at most 8
    launches and read-backs (degrees, the longest row, the delimiters, the permutation).  So
        launches + read-backs <= 8 + 2 * ceil((3 n + 16) / BUDGET)
    and doubling n adds at most 2 * ceil(3 (n / 2) / BUDGET) — not n, and not the number of levels or components."""
    n = 5000 if kind == "eye" else 20000
    cost = {}
    for size in (n, n // 2):
        m = eye(size) if kind == "eye" else R.from_edges(size, path(size))
        o = _order(_mat(m), R.PSEUDO_PERIPHERAL, R.REVERSED)
        _same(o, R.cuthill_mckee(m, R.PSEUDO_PERIPHERAL, R.REVERSED))
        cost[size] = o.stats["launches"] + o.stats["readbacks"]
        assert cost[size] <= 8 + 2 * math.ceil((3 * size + 16) / BUDGET), (size, o.stats)
        assert o.stats["levels"] == size
    assert cost[n] - cost[n // 2] <= 2 * math.ceil(3 * (n // 2) / BUDGET), cost


# ---- 6. PseudoPeripheral ---------------------------------------------------------------------------------------------------------

def test_pseudo_peripheral_swaps_and_contender_tie():
    _check_all(two_swap_graph())
    _check_all(contender_tie_graph()[0])
    _check_all(R.from_edges(30, path(30)), caps=(None, 8, 0), pairs=[(R.PSEUDO_PERIPHERAL, R.REVERSED), (R.PSEUDO_PERIPHERAL, R.FORWARD)])


# ---- 7. degrees, max_outer_nnz ---------------------------------------------------------------------------------------------------

def _with_diagonal(m):
    shape, ip, ix, dt = m
    rows = [set(np.asarray(ix[int(ip[r]):int(ip[r + 1])]).astype(np.int64).tolist()) for r in range(shape[0])]
    for r in range(0, min(shape), 2):
        rows[r].add(r)
    ip2 = np.zeros(shape[0] + 1, dtype=np.int64)
    ix2 = []
    for r in range(shape[0]):
        ix2 += sorted(rows[r])
        ip2[r + 1] = len(ix2)
    return shape, ip2, np.array(ix2, dtype=np.int64), np.ones(len(ix2))


@pytest.mark.parametrize("idx,ptr", WIDTHS)
@pytest.mark.parametrize("storage", [CSR, CSC])
def test_degrees_and_max_outer_nnz(storage, idx, ptr):
    hub = 2500 if EMULATED else 5000
    lens = [0, 3, 0, 0, 7, 1, hub, 0, 2, 64, 65, 0, 33, 1, 0]
    cols = 6000
    base = ragged_csr(lens, cols, seed=4)
    for m in (base, _with_diagonal(base)):
        shape = m[0] if storage == CSR else (m[0][1], m[0][0])
        a = _mat((shape, m[1], m[2], m[3]), storage, idx, ptr)
        assert a.degrees().tolist() == R.degrees(m)
        assert a.max_outer_nnz() == R.max_outer_nnz(m) >= hub
    z = _mat(((0, 0), [0], [], []), storage, idx, ptr)
    assert z.degrees().tolist() == [] and z.max_outer_nnz() == 0
    e = _mat(((4, 4), [0, 0, 0, 0, 0], [], []), storage, idx, ptr)
    assert e.degrees().tolist() == [0, 0, 0, 0] and e.max_outer_nnz() == 0


# ---- 8. is_symmetric -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("storage", [CSR, CSC])
def test_is_symmetric(fx, storage):
    from sprs_amd import ordering as O
    shape, ip, ix, dt = as_csr(fx["is_symmetric_simple"])
    up = lambda d, i=ix, p=ip, s=shape: _mat((s, p, i, d), storage)
    assert O.is_symmetric(up(dt))
    ulp = dt.copy()
    ulp[1] = np.nextafter(ulp[1], 1.0)               # (0, 8) against (8, 0), one ulp apart
    assert not O.is_symmetric(up(ulp)) and not R.is_symmetric((shape, ip, ix, ulp))
    nan = dt.copy()
    nan[0] = np.nan                                  # on the diagonal
    assert not O.is_symmetric(up(nan))
    zeros = dt.copy()
    zeros[1], zeros[20] = -0.0, 0.0                  # (0, 8) = -0.0, (8, 0) = 0.0
    assert O.is_symmetric(up(zeros)) and R.is_symmetric((shape, ip, ix, zeros))
    assert not O.is_symmetric(_mat(((2, 3), [0, 1, 2] if storage == CSR else [0, 1, 2, 2], [0, 1], [1.0, 1.0]), storage))
    # a hub row (longer than a tile) with one mirror entry missing
    n = 3000 if EMULATED else 6000
    s = star(n - 1)
    assert O.is_symmetric(_mat(s, storage))
    shape, ip, ix, dt = s
    k = int(ip[n // 2])                              # row n / 2 = [0, n / 2]: drop its entry 0
    ix2, dt2, ip2 = np.delete(ix, k), np.delete(dt, k), ip.copy()
    ip2[n // 2 + 1:] -= 1
    assert not O.is_symmetric(_mat((shape, ip2, ix2, dt2), storage))
    assert O.is_symmetric(_mat(((0, 0), [0], [], []), storage))


# ---- 9. contracts ----------------------------------------------------------------------------------------------------------------

def test_contracts():
    from sprs_amd import SprsHipError, _ffi
    from sprs_amd import ordering as O
    with pytest.raises(SprsHipError) as e:
        O.reverse_cuthill_mckee(_mat(((2, 3), [0, 1, 2], [0, 1], [1.0, 1.0])))
    assert e.value.status == _ffi.DIM_MISMATCH and "assertion `left == right` failed" in str(e.value) and "left: 3" in str(e.value)
    directed = R.from_edges(6, [(0, 3), (3, 1), (1, 5), (2, 4)], diag=True, symmetric=False)
    a = _mat(directed)
    with pytest.raises(SprsHipError) as e:
        O.reverse_cuthill_mckee(a, check_symmetric=True)
    assert e.value.status == _ffi.BAD_STRUCTURE and str(e.value).endswith("matrix is not symmetric")
    z = O.reverse_cuthill_mckee(_mat(((0, 0), [0], [], [])))
    assert z.perm.vec().tolist() == [] and z.connected_parts.tolist() == [0] and z.dim == 0
    with pytest.raises(SprsHipError) as e:
        O.cuthill_mckee_custom(a, 7, 0)
    assert e.value.status == _ffi.INVALID_ARG


@pytest.mark.parametrize("seed", range(12))
def test_non_symmetric_patterns_without_the_check(seed):
    """what the sequential loop gives on the directed pattern — including its panic when the pseudo-peripheral search hands
    back a vertex of an earlier component (ordering.rs:488-491)"""
    from sprs_amd import SprsHipError, _ffi
    m = R.random_pattern(5 + 6 * seed, 400 + seed, False, density=1.0)
    a = _mat(m)
    for strategy, direction in PAIRS:
        for cap in (1024, 8, 0):
            try:
                want = R.cuthill_mckee(m, strategy, direction)
            except R.StartVisited as err:
                with pytest.raises(SprsHipError) as e:
                    _order(a, strategy, direction, cap)
                assert e.value.status == _ffi.BAD_STRUCTURE and str(err) in str(e.value)
                continue
            _same(_order(a, strategy, direction, cap), want)


# ---- 10. end to end --------------------------------------------------------------------------------------------------------------

def test_fill_in_reduction_end_to_end():
    """examples/fill_in_reduction.rs with both steps on the device"""
    from sprs_amd import ordering as O
    from sprs_amd import permutation as P
    side = 16 if EMULATED else 64
    m = grid_laplacian(side, side, shuffle_seed=9)
    a = _mat(m)
    o = O.reverse_cuthill_mckee(a, check_symmetric=True)
    perm, parts = R.reverse_cuthill_mckee(m)
    _same(o, (perm, parts))
    got = P.transform_mat_papt(a, o.perm).to_host()
    want = perm_ref.transform_mat_papt_vec(m, CSR, perm)
    assert perm_ref.same_mat(got, want)
    assert R.bandwidth(got) == R.bandwidth(want) < R.bandwidth(m)


@large
def test_callers_non_blocking_stream():
    torch = pytest.importorskip("torch")
    from sprs_amd import ordering as O
    m = grid_laplacian(64, 64, shuffle_seed=3)
    a = _mat(m)
    st = torch.cuda.Stream()
    for strategy, direction in PAIRS:
        _same(O.cuthill_mckee_custom(a, strategy, direction, stream=st), R.cuthill_mckee(m, strategy, direction))
    assert O.is_symmetric(a, stream=st)
    assert a.degrees(stream=st).tolist() == R.degrees(m) and a.max_outer_nnz(stream=st) == 5
    small = grid_laplacian(20, 20, shuffle_seed=4)      # wide levels on the caller's stream
    _same(_order(_mat(small), R.PSEUDO_PERIPHERAL, R.REVERSED, 8, stream=st), R.reverse_cuthill_mckee(small))


@large
def test_cpp_mirror():
    """include/sprs_hip.hpp (namespace ordering, DeviceCsMat::degrees / max_outer_nnz) through the same C ABI"""
    import subprocess
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = os.path.join(cpp, "ordering_mirror_test.bin")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", cpp, "-f", "ordering_mirror.mk"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all passed" in r.stdout, r.stdout + r.stderr
