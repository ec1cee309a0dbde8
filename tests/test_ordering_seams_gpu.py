"""Device orderings at the limits of the one-workgroup kernel and at the tile seams of the nnz-tiled kernels (ordering.hpp): the
entry limit of a narrow level (OD_NARROW_ENTRIES), the LDS sort at 512 .. 4096 slots and more candidates than OD_NARROW_MAX, a
frontier of exactly the cap, wide levels of thousands with both sort routes and an entry count at a multiple of OD_TILE, the step
at which the machine is stopped and resumed (OD_BUDGET), directed patterns at size, and degrees / max_outer_nnz / is_symmetric
where a tile meets more than OD_ROWS slices, where the longest row sits in the second OD_CHUNK and where the offender is at a
tile's edge.  Everything is compared for exact equality with the restatement tests/ordering_ref.py.

THE ROUTE WITNESS.  stats["launches"] and stats["readbacks"] are counted by host code.  A call costs
    2 launches + 1 read-back   degrees (lengths, diagonal) and the longest row
    2 launches                 MinimumDegree only: the vertices by degree (keys, sort)
    1 launch + 1 read-back     per launch of the one-workgroup kernel
    1 launch, 1 read-back      the permutation; the delimiters
so a call WITHOUT a wide level has launches - readbacks == 1 (3 under MinimumDegree).  A wide level adds lengths, scan [+ expand
[+ keys and sort (packed key; 3 more on the two-pass route), copy]] and one read-back each for the entry and the candidate count:
(2, 1), (3, 2), (5, 2) or (7, 2) — always more launches than read-backs.  Handing a level over costs nothing: the launch that
stops with WHY_WIDE is the one that would have run the level.  So
    launches - readbacks > 1 (3)     <=>  at least one level ran wide
    a level with candidates that moves from narrow to wide on the packed route adds exactly 5 launches and 2 read-backs
Each seam case asserts one of the two, or a precondition computed from its input, so that it fails when a constant moves away
from under it.

The cases not marked `large` also run against the kernel emulator (tests/test_ordering_emu_cpu.py)."""
import functools
import os
import re

import numpy as np
import pytest

import ordering_ref as R
from conftest import ROOT
from test_ordering_gpu import (CSC, CSR, EMULATED, PAIRS, WIDTHS, _default_options, _mat, _need_device, _order,  # noqa: F401
                               _same, eye, large, path, star)

pytestmark = pytest.mark.gpu

# The kernels' constants, read from the source: the sizes below are literal, so a constant that moves away from under a case fails
# that case's precondition instead of leaving it green beside the seam.
with open(os.path.join(ROOT, "sprs_amd", "csrc", "ordering.hpp")) as _f:
    OD = {k: int(v) for k, v in re.findall(r"constexpr (?:int|uint64_t) (OD_[A-Z_]+) = (\d+);", _f.read())}
CAP = OD["OD_NARROW_MAX"]                           # 1024, the default ordering_narrow_cap
ENTRIES = OD["OD_NARROW_ENTRIES"]                   # 4096
TILE = OD["OD_TILE"]                                # 2048
ROWS = OD["OD_ROWS"]                                # 2048
CHUNK = OD["OD_CHUNK"]                              # 8192
BUDGET = OD["OD_BUDGET"]                            # 16384 steps per launch
NEXT_FWD = (R.NEXT, R.FORWARD)


# ---- generators ------------------------------------------------------------------------------------------------------------------

def tree2(fan, kids, extra=0, seed=None):
    """Vertex 0 is the root, 1 .. fan its children, then `kids` leaves per child (`kids + extra` for the last one), the diagonal
    stored: a child's row holds kids + 2 entries, the children's level fan * (kids + 2) + extra entries and fan * kids + extra
    candidates.  With a seed the vertices are renumbered by a permutation."""
    edges = [(0, c) for c in range(1, fan + 1)]
    leaf = fan + 1
    for c in range(1, fan + 1):
        for _ in range(kids + (extra if c == fan else 0)):
            edges.append((c, leaf))
            leaf += 1
    if seed is not None:
        p = np.random.default_rng(seed).permutation(leaf).tolist()
        edges = [(p[i], p[j]) for i, j in edges]
    return R.from_edges(leaf, edges)


def path_graph(n, start_at=0):
    """a path of n; vertex 0 sits `start_at` places from its end (it trades names with the vertex there)"""
    name = {0: start_at, start_at: 0}
    return R.from_edges(n, [(name.get(i, i), name.get(j, j)) for i, j in path(n)])


def random_symmetric(n, seed, density):
    return R.random_pattern(n, seed, True, density)


def random_directed(n, seed, density):
    return R.random_pattern(n, seed, False, density)


MAKERS = {"tree2": tree2, "star": star, "eye": eye, "path": path_graph, "sym": random_symmetric, "directed": random_directed}


@functools.lru_cache(maxsize=None)
def _graph(kind, *args):
    return MAKERS[kind](*args)


@functools.lru_cache(maxsize=None)
def _want(strategy, direction, kind, *args):
    """the restatement's answer, computed once per (graph, strategy, direction); StartVisited is returned, not raised"""
    try:
        return R.cuthill_mckee(_graph(kind, *args), strategy, direction)
    except R.StartVisited as err:
        return err


def _run(case, strategy, direction, cap=CAP):
    o = _order(_mat(_graph(*case)), strategy, direction, cap)
    _same(o, _want(strategy, direction, *case))
    return o


def _all_pairs(case):
    a = _mat(_graph(*case))
    for strategy, direction in PAIRS:
        _same(_order(a, strategy, direction, CAP), _want(strategy, direction, *case))


def _net(o, strategy=R.NEXT):
    """launches - read-backs above those of a call without a wide level: 0 <=> no level ran wide (see the module's docstring)"""
    return o.stats["launches"] - o.stats["readbacks"] - (3 if strategy == R.MINIMUM_DEGREE else 1)


def _witness(narrow_case, wide_case, levels):
    """the same graph but for one level that is narrow on one side and wide on the other, under start.Next, order.Forward, the
    default cap and 64-bit keys: that level has candidates, so the wide side costs 5 launches and 2 read-backs more"""
    nar, wid = _run(narrow_case, *NEXT_FWD), _run(wide_case, *NEXT_FWD)
    assert nar.stats["levels"] == wid.stats["levels"] == levels, (nar.stats, wid.stats)
    assert wid.stats["launches"] - nar.stats["launches"] == 5, (nar.stats, wid.stats)
    assert wid.stats["readbacks"] - nar.stats["readbacks"] == 2, (nar.stats, wid.stats)


def _level_entries(m, first, last):
    """stored entries of the rows first .. last"""
    ip = np.asarray(m[1]).astype(np.int64)
    return int(ip[last + 1] - ip[first])


# ---- 1. the entry limit of a narrow level ----------------------------------------------------------------------------------------

ENTRY_PAIRS = [
    # (narrow side, wide side, levels, entries of the level on the narrow side, its candidates)
    (("star", 4094), ("star", 4096), 2, 4095, 4094),
    (("star", 4095), ("star", 4096), 2, 4096, 4095),
    (("tree2", 1024, 2), ("tree2", 1024, 2, 1), 3, 4096, 2048),
    (("tree2", 512, 6), ("tree2", 512, 6, 1), 3, 4096, 3072),
    (("tree2", 2, 2046), ("tree2", 2, 2047), 3, 4096, 4092),
]


@pytest.mark.parametrize("narrow,wide,levels,entries,cands", ENTRY_PAIRS, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else None)
def test_entry_limit_of_a_narrow_level(narrow, wide, levels, entries, cands):
    """A frontier whose rows hold exactly OD_NARROW_ENTRIES entries (or one less) stays in the one-workgroup kernel, one entry
    more hands it over.  The level is the centre's row of a star, or the children of a tree2: on the narrow side it has 2048 ..
    4095 candidates, so the LDS sort runs at 2048 and 4096 slots, s_front is left unfilled (more than OD_NARROW_MAX candidates),
    and the level after it is wider than the cap: it goes wide from the same launch."""
    star_like = narrow[0] == "star"
    rows = (0, 0) if star_like else (1, narrow[1])
    assert _level_entries(_graph(*narrow), *rows) == entries <= ENTRIES < _level_entries(_graph(*wide), *rows) <= ENTRIES + 2
    assert CAP < cands <= ENTRIES and rows[1] - rows[0] + 1 <= CAP
    _witness(narrow, wide, levels)
    _all_pairs(narrow)
    _all_pairs(wide)


# ---- 2. the frontier's length at the cap -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("fan", [1023, 1024])
def test_frontier_length_at_the_cap(fan):
    """1023 and 1024 children are a narrow level at the default cap (4092 and 4096 entries), 1025 are handed over for their
    length alone"""
    assert _level_entries(_graph("tree2", fan, 2), 1, fan) <= ENTRIES and fan <= CAP < 1025
    _witness(("tree2", fan, 2), ("tree2", 1025, 2), 3)
    _all_pairs(("tree2", fan, 2))
    _all_pairs(("tree2", 1025, 2))


@pytest.mark.parametrize("fan", [1023, 1024, 1025])
def test_frontier_length_at_the_cap_renumbered(fan):
    """the same trees with their vertices renumbered: the start vertex is not the root, the levels differ per strategy"""
    case = ("tree2", fan, 2, 0, 5 + fan)
    assert int(_graph(*case)[1][1]) < fan            # vertex 0, where start.Next begins, is not the root (fan + 1 entries)
    _all_pairs(case)


# ---- 3. the sort sizes in between ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fan", [511, 512, 513, 1023])
def test_sort_sizes_in_between(fan):
    """fan candidates in the root's level and again in the children's: the LDS sort at 512 and 1024 slots, at the slot count and
    one either side.  No level is wider than the cap or holds more than 3 * 1023 entries: the whole call stays narrow."""
    case = ("tree2", fan, 1)
    assert fan <= CAP and _level_entries(_graph(*case), 1, fan) == 3 * fan <= ENTRIES
    o = _run(case, *NEXT_FWD)
    assert _net(o) == 0 and o.stats["levels"] == 3, o.stats
    _all_pairs(case)


# ---- 4. wide levels of natural size ----------------------------------------------------------------------------------------------

NATURAL = [("sym", 3000, 41, 2.0), ("sym", 6000, 42, 1.5), ("sym", 5000, 43, 4.0)]
TWO_STRATEGIES = [(R.PSEUDO_PERIPHERAL, R.REVERSED), (R.MINIMUM_DEGREE, R.FORWARD)]


@pytest.mark.parametrize("cap", [1024, 100])
@pytest.mark.parametrize("case", NATURAL, ids=lambda c: "n%d-d%s" % (c[1], c[3]))
def test_wide_levels_of_natural_size(case, cap):
    """random patterns of thousands: narrow and wide levels mixed, the packed-key sort on levels of thousands"""
    for strategy, direction in TWO_STRATEGIES:
        o = _run(case, strategy, direction, cap)
        print(case, cap, strategy, o.stats)
        assert _net(o, strategy) > 0, o.stats        # more launches than the same call without a wide level


def _with_key_bits(bits, fn):
    import sprs_amd
    sprs_amd.set_option("ordering_key_bits", bits)
    try:
        return fn()
    finally:
        sprs_amd.set_option("ordering_key_bits", 64)


@pytest.mark.parametrize("cap", [1024, 8])
@pytest.mark.parametrize("case", [NATURAL[0], ("star", 5000), ("tree2", 1025, 2, 0, 1030)], ids=lambda c: "-".join(map(str, c)))
def test_two_pass_sort_route_on_levels_of_thousands(case, cap):
    """ordering_key_bits = 1: every wide level with candidates sorts by id, then stably by (owner, degree).  Under start.Next the
    star's only level with candidates is the centre's (5001 entries: wide at every cap): the two-pass route costs exactly 2
    launches more than the packed one and no read-back."""
    for strategy, direction in PAIRS:
        o = _with_key_bits(1, lambda: _run(case, strategy, direction, cap))
        assert _net(o, strategy) > 0, o.stats
    if case[0] == "star":
        two = _with_key_bits(1, lambda: _run(case, *NEXT_FWD, cap))
        one = _run(case, *NEXT_FWD, cap)
        assert two.stats["launches"] - one.stats["launches"] == 2 and two.stats["readbacks"] == one.stats["readbacks"], (one.stats, two.stats)


@pytest.mark.parametrize("extra,entries", [(1, 2 * TILE), (2, 2 * TILE + 1)])
def test_wide_level_at_a_multiple_of_the_tile(extra, entries):
    """1365 children (more than the cap: a wide level) of one leaf, the last with `extra` more: 3 * 1365 + extra entries, exactly
    two tiles of the expand kernel, and one entry into a third"""
    case = ("tree2", 1365, 1, extra)
    assert 1365 > CAP and _level_entries(_graph(*case), 1, 1365) == entries
    o = _run(case, *NEXT_FWD)
    assert _net(o) > 0 and o.stats["levels"] == 3, o.stats
    _all_pairs(case)


# ---- 5. the budget seam ----------------------------------------------------------------------------------------------------------

def _budget_pair(n):
    for strategy, direction in (NEXT_FWD, (R.PSEUDO_PERIPHERAL, R.REVERSED)):
        a, b = _run(("eye", n), strategy, direction), _run(("eye", n + 1), strategy, direction)
        assert _net(a) == _net(b) == 0
        assert a.stats["launches"] == 3 + -(-(3 * n + 1) // BUDGET), a.stats       # (the module's docstring)
        assert b.stats["launches"] - a.stats["launches"] == 1 and b.stats["readbacks"] - a.stats["readbacks"] == 1, (a.stats, b.stats)


def test_budget_seam_second_launch():
    """eye(n) takes 3 n + 1 steps (a start vertex, its level, the end of its search; the closing delimiter): 5461 vertices are
    exactly OD_BUDGET steps, 5462 stop the machine and resume it — one launch and one read-back more"""
    assert 3 * 5461 + 1 == BUDGET < 3 * 5462 + 1
    _budget_pair(5461)


@large
def test_budget_seam_third_launch():
    assert 3 * 10922 + 1 <= 2 * BUDGET < 3 * 10923 + 1
    _budget_pair(10922)


@pytest.mark.parametrize("start_at", [0, 1500])
def test_budget_cuts_the_pseudo_peripheral_search(start_at):
    """A path of 6000 under the pseudo-peripheral search.  From its end: two level structures of 6000 levels (equal heights, no
    swap) and the order, 3 * 6001 + 1 steps, so the first launch ends inside the order.  From 1500 places off the end: a structure
    of 4500 levels, one of 6000 from the far end (higher: swap), one of 6000 from the near end, then the order: the first launch
    ends 120 levels before the end of the third structure, mid-search, and the second inside the order."""
    n = 6000
    steps = 3 * (n + 1) + 1 if start_at == 0 else 1 + (n - start_at + 1) + 3 * (n + 1)
    assert steps - (n + 1) < BUDGET < steps if start_at == 0 else steps - 2 * (n + 1) < BUDGET < steps - (n + 1)
    trace = []
    R.cuthill_mckee(_graph("path", n, start_at), R.PSEUDO_PERIPHERAL, R.REVERSED, trace)
    assert trace == [1 if start_at else 0]                                           # the swaps of the George-Liu loop
    for direction in (R.REVERSED, R.FORWARD):
        o = _run(("path", n, start_at), R.PSEUDO_PERIPHERAL, direction)
        assert _net(o) == 0 and o.stats["levels"] == n, o.stats


# ---- 6. non-symmetric patterns at size -------------------------------------------------------------------------------------------

def _levels_next(m):
    """(vertices, stored entries) of every level of the ordering under start.Next, from the pattern alone"""
    rows = R._rows(m)
    seen = [False] * len(rows)
    out = []
    for v in range(len(rows)):
        if not seen[v]:
            out += [(len(lv), sum(len(rows[j]) for j in lv)) for lv in R._levels(v, rows, seen, lambda pos, j: (pos, j))]
    return out


@pytest.mark.parametrize("n,seed,density", [(3000, 100, 2.0), (3000, 101, 2.0), (6000, 102, 3.0)])
def test_non_symmetric_patterns_at_size(n, seed, density):
    """directed patterns of thousands without the symmetry check: what the sequential loop gives, including its panic under the
    pseudo-peripheral search (ordering.rs:488-491).  The levels of the patterns of 3000 stay below 500 vertices and 1400 entries:
    they go wide at a cap of 64 only; the pattern of 6000 has levels that go wide at the default cap."""
    from sprs_amd import SprsHipError, _ffi
    case = ("directed", n, seed, density)
    a = _mat(_graph(*case))
    levels = _levels_next(_graph(*case))
    goes_wide = {cap: any(f > cap or e > ENTRIES for f, e in levels) for cap in (1024, 64)}
    print(case, "longest level", max(f for f, e in levels), "most entries", max(e for f, e in levels), goes_wide)
    assert goes_wide[64] and goes_wide[1024] == (n == 6000)
    outcomes = set()
    for strategy in R.STRATEGIES:
        want = _want(strategy, R.FORWARD, *case)
        for cap in (1024, 64):
            if isinstance(want, R.StartVisited):
                with pytest.raises(SprsHipError) as e:
                    _order(a, strategy, R.FORWARD, cap)
                assert e.value.status == _ffi.BAD_STRUCTURE and str(want) in str(e.value)
                outcomes.add("panic")
                continue
            o = _order(a, strategy, R.FORWARD, cap)
            _same(o, want)
            outcomes.add("order")
            if strategy == R.NEXT:
                assert (_net(o) > 0) == goes_wide[cap], (o.stats, cap)
    assert outcomes == {"panic", "order"}


# ---- 7. degrees, max_outer_nnz, is_symmetric on sparse slice starts --------------------------------------------------------------

def _symmetric_values(m):
    """one value per unordered pair, exact in f64 and different between neighbouring pairs"""
    shape, ip, ix, _ = m
    rows = np.repeat(np.arange(shape[0]), np.diff(ip))
    lo, hi = np.minimum(rows, ix), np.maximum(rows, ix)
    return shape, ip, ix, 1.0 + ((7 * lo + 13 * hi) % 4093) / 4096.0


@functools.lru_cache(maxsize=None)
def sparse_starts():
    """n = 9001, stored entries only on the rows and columns that are multiples of 4: their diagonal, 1500 random mirrored pairs
    and the hub 8600 joined to all of them"""
    n, hub = 9001, 8600
    rng = np.random.default_rng(2024)
    live = np.arange(0, n, 4)
    edges = [(int(v), int(v)) for v in live] + [(hub, int(v)) for v in live]
    edges += [(int(i), int(j)) for i, j in rng.choice(live, size=(1500, 2)) if i != j]
    return _symmetric_values(R.from_edges(n, edges, diag=False))


@functools.lru_cache(maxsize=None)
def strided(stride, live, hub=None, shift_from=None):
    """`live` rows, at the multiples of `stride` (from the live row `shift_from` on: stride - 1 rows later), of exactly 4 entries:
    the diagonal, the live rows before and after (cyclically) and the one half-way round; everything else empty.  Or, with `hub`,
    only the diagonal of the live rows and that hub row."""
    at = [stride * i + (stride - 1 if shift_from is not None and i >= shift_from else 0) for i in range(live)]
    edges = [(v, v) for v in at]
    if hub is None:
        assert live % 2 == 0
        edges += [(at[i], at[(i + 1) % live]) for i in range(live)] + [(at[i], at[(i + live // 2) % live]) for i in range(live)]
    else:
        edges += [(hub, v) for v in at]
    return _symmetric_values(R.from_edges(at[-1] + 1, edges, diag=False))


def _row_of(ip, k):
    return int(np.searchsorted(np.asarray(ip).astype(np.int64), k, side="right")) - 1


def _tile_slices(m):
    """per tile of OD_TILE entries, the slices it meets: from the last one that starts at or before its first entry to the last one
    that starts at or before its last entry (stage_tile_rows)"""
    shape, ip, ix, _ = m
    out = []
    for k0 in range(0, ix.size, TILE):
        k1 = min(k0 + TILE, ix.size)
        out.append(min(_row_of(ip, k1 - 1), shape[0] - 1) - min(_row_of(ip, k0), shape[0] - 1) + 1)
    return out


def _drop(m, k, diagonal=False):
    shape, ip, ix, dt = m
    assert (int(ix[k]) == _row_of(ip, k)) == diagonal
    ip2 = np.array(ip, dtype=np.int64)
    ip2[_row_of(ip, k) + 1:] -= 1
    return shape, ip2, np.delete(ix, k), np.delete(dt, k)


def _mirror(m, k):
    """the position of the entry (c, r) for the entry (r, c) at position k"""
    shape, ip, ix, _ = m
    r, c = _row_of(ip, k), int(ix[k])
    s, e = int(ip[c]), int(ip[c + 1])
    at = s + int(np.searchsorted(ix[s:e], r))
    assert at < e and int(ix[at]) == r
    return at


@functools.lru_cache(maxsize=None)
def _facts(key):
    """(degrees, max_outer_nnz, is_symmetric) of the restatement, once per matrix"""
    m = DERIVED[key]()
    return R.degrees(m), R.max_outer_nnz(m), R.is_symmetric(m)


def _check_three(key, storage, idx, ptr):
    from sprs_amd import ordering as O
    m = DERIVED[key]()
    deg, longest, sym = _facts(key)
    a = _mat(m, storage, idx, ptr)
    assert a.degrees().tolist() == deg
    assert a.max_outer_nnz() == longest
    assert O.is_symmetric(a) == sym
    return deg, longest, sym


def _tile_edge(m, last, offends=False):
    """-> (k, the position to drop): k is the first position of a tile other than tile 0 (the last position of a full tile, with
    `last`) that holds an off-diagonal entry.  Without `offends` that entry is dropped.  With it, the mirror of the entry that
    stands at k AFTERWARDS is dropped, so that k is where the one offender is: the entry at k when its mirror lies behind it, the
    one at k + 1 when its mirror lies in front of both."""
    shape, ip, ix, _ = m
    for t in range(1, ix.size // TILE):
        k = t * TILE + (TILE - 1 if last else 0)
        if not offends and int(ix[k]) != _row_of(ip, k):
            return k, k
        for q in (k, k + 1) if offends else ():
            if int(ix[q]) != _row_of(ip, q) and (_mirror(m, q) > q) == (q == k) and (q == k or _mirror(m, q) < k):
                return k, _mirror(m, q)
    raise AssertionError("no tile edge with a suitable entry")


def _hub_entry(m):
    shape, ip, ix, _ = m
    k = int(ip[8600]) + 1000
    assert _row_of(ip, k) == 8600 and int(ix[k]) != 8600
    return k


def _one_ulp_in_the_last_tile(m):
    shape, ip, ix, dt = m
    k = (ix.size - 1) // TILE * TILE + 5
    assert k < ix.size and int(ix[k]) != _row_of(ip, k)
    dt2 = dt.copy()
    dt2[k] = np.nextafter(dt2[k], 4.0)
    return shape, ip, ix, dt2


def _diagonal_of(m, r):
    shape, ip, ix, _ = m
    k = int(ip[r]) + int(np.searchsorted(ix[int(ip[r]):int(ip[r + 1])], r))
    assert _row_of(ip, k) == r and int(ix[k]) == r
    return k


DERIVED = {
    "whole": sparse_starts,
    # the entry at a tile's edge dropped: its mirror, elsewhere, is the offender
    "first-of-tile": lambda: _drop(sparse_starts(), _tile_edge(sparse_starts(), False)[1]),
    "last-of-tile": lambda: _drop(sparse_starts(), _tile_edge(sparse_starts(), True)[1]),
    # the mirror of another entry dropped, so that the entry left without one stands AT the tile's edge: the only offender
    "first-of-tile-offends": lambda: _drop(sparse_starts(), _tile_edge(sparse_starts(), False, True)[1]),
    "last-of-tile-offends": lambda: _drop(sparse_starts(), _tile_edge(sparse_starts(), True, True)[1]),
    "hub-entry": lambda: _drop(sparse_starts(), _hub_entry(sparse_starts())),
    "one-ulp": lambda: _one_ulp_in_the_last_tile(sparse_starts()),
    "diagonal": lambda: _drop(sparse_starts(), _diagonal_of(sparse_starts(), 4000), diagonal=True),
    "hub-diagonal": lambda: _drop(sparse_starts(), _diagonal_of(sparse_starts(), 8600), diagonal=True),
    "edges-4": lambda: strided(4, 1536),
    "edges-4-dropped": lambda: _drop(strided(4, 1536), TILE + 2),
    "edges-4-exact": lambda: strided(4, 1536, None, 511),
    "edges-4-exact-dropped": lambda: _drop(strided(4, 1536, None, 511), TILE - 1),
    "edges-8": lambda: strided(8, 1024),
    "edges-8-dropped": lambda: _drop(strided(8, 1024), 2 * TILE - 2),
    "hub-8192": lambda: strided(4, 2049, hub=8192),
    "hub-8191": lambda: strided(4, 2049, hub=8191),
}


def test_sparse_starts_preconditions():
    """what makes the cases below meaningful, computed from the matrices"""
    m = sparse_starts()
    shape, ip, ix, dt = m
    lens = np.diff(ip)
    assert shape == (9001, 9001) and max(_tile_slices(m)) > ROWS                 # the unstaged slice search runs
    assert int(np.argmax(lens)) == 8600 > CHUNK and int(lens[8600]) == 2251      # the longest row is in the second workgroup
    assert np.count_nonzero(lens == lens.max()) == 1 and int(lens[:CHUNK].max()) < 2251
    assert ix.size > 4 * TILE and not np.any(lens[np.arange(9001) % 4 != 0])
    for key, last in (("first-of-tile", False), ("last-of-tile", True)):
        k, dropped = _tile_edge(m, last)
        assert k == dropped >= TILE and k % TILE == (TILE - 1 if last else 0) and int(ix[k]) != _row_of(ip, k)   # off the diagonal
        k, dropped = _tile_edge(m, last, offends=True)
        d = DERIVED[key + "-offends"]()
        r, c = _row_of(d[1], k), int(d[2][k])        # the entry at the tile's edge has no mirror, every other entry has one
        assert k >= TILE and k % TILE == (TILE - 1 if last else 0) and r != c and r not in d[2][int(d[1][c]):int(d[1][c + 1])].tolist()
        assert d[2].size == ix.size - 1 and int(ix[dropped]) == r and _row_of(ip, dropped) == c
    for stride, live in ((4, 1536), (8, 1024)):
        s = strided(stride, live)
        assert set(np.diff(s[1])[::stride].tolist()) == {TILE // 512} and s[2].size % TILE == 0
        assert all(int(s[1][_row_of(s[1], k)]) == k for k in range(0, s[2].size, TILE))    # tile edges are slice edges
        assert (max(_tile_slices(s)) > ROWS) == (stride == 8)
    # exactly OD_ROWS slices in a tile (the last that are staged) and one more (the first that are not)
    assert _tile_slices(DERIVED["edges-4-exact"]())[0] == ROWS and ROWS + 1 in _tile_slices(DERIVED["edges-4-dropped"]())
    for hub in (8192, 8191):
        h = strided(4, 2049, hub=hub)
        lens = np.diff(h[1])
        assert h[0] == (8193, 8193) and int(np.argmax(lens)) == hub and np.count_nonzero(lens > 2) == 1 and (hub >= CHUNK) == (hub == 8192)


@pytest.mark.parametrize("idx,ptr", WIDTHS)
@pytest.mark.parametrize("storage", [CSR, CSC])
def test_sparse_starts_whole(storage, idx, ptr):
    assert np.iinfo(idx).max >= 9001 and np.iinfo(ptr).max >= sparse_starts()[2].size
    deg, longest, sym = _check_three("whole", storage, idx, ptr)
    assert sym and longest == 2251 and deg[8600] == 2250


@pytest.mark.parametrize("storage", [CSR, CSC])
@pytest.mark.parametrize("key", ["first-of-tile", "last-of-tile", "first-of-tile-offends", "last-of-tile-offends", "hub-entry", "one-ulp"])
def test_sparse_starts_one_offender(key, storage):
    """one entry without its mirror, or one value one ulp off: not symmetric; degrees and the longest row as the restatement has them"""
    for idx, ptr in (WIDTHS[0], WIDTHS[-1]):
        deg, longest, sym = _check_three(key, storage, idx, ptr)
        assert not sym
        assert sum(deg) == sum(_facts("whole")[0]) - (0 if key == "one-ulp" else 1)


@pytest.mark.parametrize("storage", [CSR, CSC])
def test_sparse_starts_without_a_diagonal_entry(storage):
    """a stored diagonal entry is not a neighbour and is its own mirror: symmetric still, degrees unchanged; the longest row is
    one shorter only where it was the hub's"""
    whole = _facts("whole")
    for key, longest in (("diagonal", 2251), ("hub-diagonal", 2250)):
        assert _check_three(key, storage, *WIDTHS[0]) == (whole[0], longest, True)


@pytest.mark.parametrize("storage", [CSR, CSC])
@pytest.mark.parametrize("key", ["edges-4", "edges-4-exact", "edges-8", "hub-8192", "hub-8191"])
def test_tile_and_chunk_edges_on_slice_edges(key, storage):
    """rows of exactly 4 entries at every 4th (8th) row: every tile begins at a slice's first entry behind a run of empty rows,
    staged (2045 slices) and unstaged (4089); with one live row moved, a tile of exactly OD_ROWS slices, and with one entry
    dropped, one of OD_ROWS + 1.  And the only long row in the first row of the second chunk of rows, or the last
    of the first."""
    for idx, ptr in (WIDTHS[0], WIDTHS[-1]):
        deg, longest, sym = _check_three(key, storage, idx, ptr)
        assert sym and longest == (4 if key.startswith("edges") else 2049)
        if key.startswith("edges"):
            assert not _check_three(key + "-dropped", storage, idx, ptr)[2]
