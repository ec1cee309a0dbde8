"""The oracle of the ordering tests checks itself: tests/ordering_ref.py reproduces the reference's own test data
(tests/golden/ordering_fixtures.json, from ordering.rs:567-660 and symmetric.rs:42-57), and its two formulations — the
sequential deque loop, line by line from ordering.rs, and the level-by-level form the device kernels implement — agree on random
symmetric and non-symmetric patterns, for the three start strategies and both directions."""
import json
import os

import numpy as np
import pytest

import ordering_ref as R
from conftest import ROOT, as_csr


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(ROOT, "tests", "golden", "ordering_fixtures.json")) as f:
        return json.load(f)


def eye(n):
    return (n, n), np.arange(n + 1), np.arange(n), np.ones(n)


def test_restatement_reproduces_the_fixtures(fx):
    c = fx["unconnected_graph_lap"]
    lap = as_csr(c["mat"])
    want = c["reverse_cuthill_mckee"]
    for f in (R.reverse_cuthill_mckee, lambda m: R.cuthill_mckee_levels(m, R.PSEUDO_PERIPHERAL, R.REVERSED)):
        perm, parts = f(lap)
        assert perm == want["perm"] and parts == want["connected_parts"]
    assert R.is_symmetric(lap)
    for f in (R.cuthill_mckee, R.cuthill_mckee_levels):
        assert f(eye(3), R.PSEUDO_PERIPHERAL, R.FORWARD)[0] == fx["eye3"]["forward"]
        assert f(eye(3), R.PSEUDO_PERIPHERAL, R.REVERSED)[0] == fx["eye3"]["reversed"]
    assert R.is_symmetric(as_csr(fx["is_symmetric_simple"]))


def test_degrees_and_symmetry_of_the_restatement(fx):
    lap = as_csr(fx["unconnected_graph_lap"]["mat"])
    assert R.degrees(lap) == [3, 3, 3, 3, 3, 8, 1, 1, 3, 2, 3, 3] and R.max_outer_nnz(lap) == 9
    shape, ip, ix, dt = as_csr(fx["is_symmetric_simple"])
    dt2 = dt.copy()
    dt2[1] = np.nextafter(dt2[1], 1.0)
    assert not R.is_symmetric((shape, ip, ix, dt2))
    dt3 = dt.copy()
    dt3[0] = np.nan
    assert not R.is_symmetric((shape, ip, ix, dt3))
    assert not R.is_symmetric(((2, 3), [0, 0, 0], [], []))
    assert R.is_symmetric(((2, 2), [0, 1, 2], [1, 0], [-0.0, 0.0]))
    assert not R.is_symmetric(((2, 2), [0, 1, 1], [1], [1.0]))


def _outcome(f, m, strategy, direction):
    try:
        return f(m, strategy, direction)
    except R.StartVisited:
        return "start vertex already visited"


@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("strategy", R.STRATEGIES)
@pytest.mark.parametrize("direction", [R.FORWARD, R.REVERSED])
def test_level_form_equals_the_sequential_loop(symmetric, strategy, direction):
    panics = 0
    for seed in range(140):
        m = R.random_pattern(1 + seed % 70, 1000 + seed, symmetric)
        a, b = _outcome(R.cuthill_mckee, m, strategy, direction), _outcome(R.cuthill_mckee_levels, m, strategy, direction)
        assert a == b, (seed, a, b)
        panics += a == "start vertex already visited"
        if a != "start vertex already visited":
            perm, parts = a
            assert sorted(perm) == list(range(len(perm))) and parts[0] == 0 and parts[-1] == len(perm) and parts == sorted(set(parts))
    # the reference's assert on the start vertex can only fire on a directed pattern under the pseudo-peripheral search
    assert panics == 0 or (not symmetric and strategy == R.PSEUDO_PERIPHERAL)


def test_pseudo_peripheral_cases_swap_as_the_gpu_tests_assume():
    """the hand-made cases of tests/test_ordering_gpu.py: at least two swaps of the George-Liu loop; a contender tie whose
    order in the rooted level structure is not id order"""
    import test_ordering_gpu as G
    trace = []
    R.cuthill_mckee(G.two_swap_graph(), R.PSEUDO_PERIPHERAL, R.REVERSED, trace)
    assert max(trace) >= 2
    m, root, contender, by_id = G.contender_tie_graph()
    rows, deg = R._rows(m), R.degrees(m)
    assert R.rls_contender_and_height(root, deg, rows)[0] == contender != by_id and deg[contender] == deg[by_id]
