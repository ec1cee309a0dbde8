"""CPU restatement of sprs/src/sparse/linalg/ordering.rs for the tests, line by line: the sequential deque form of
cuthill_mckee_custom with the three start strategies and both directions, with the STABLE tie-break (vertices of equal degree
keep row order — one of the outcomes the reference's sort_unstable_by_key may give, and the one its golden permutation has).
Beside it `cuthill_mckee_levels`, an independent level-by-level formulation, and degrees / max_outer_nnz (csmat.rs:1188-1216)
and is_symmetric (symmetric.rs:7-34).

A matrix is (shape, indptr, indices, data); everything walks the OUTER dimension of the arrays, as the reference does, so the
arrays of a CSC matrix are read as they stand."""
from collections import deque

import numpy as np

NEXT, MINIMUM_DEGREE, PSEUDO_PERIPHERAL = 0, 1, 2
STRATEGIES = (NEXT, MINIMUM_DEGREE, PSEUDO_PERIPHERAL)
FORWARD, REVERSED = 0, 1


class StartVisited(AssertionError):
    """the panic of ordering.rs:488-491: on a NON-symmetric pattern the pseudo-peripheral search can walk into an earlier
    component and hand back one of its vertices"""


def _rows(m):
    shape, ip, ix, _ = m
    ip = np.asarray(ip).astype(np.int64)
    ix = np.asarray(ix).astype(np.int64)
    return [ix[ip[r]:ip[r + 1]].tolist() for r in range(len(ip) - 1)]


def max_outer_nnz(m):
    """csmat.rs:1188-1193"""
    return max((len(r) for r in _rows(m)), default=0)


def degrees(m):
    """csmat.rs:1205-1216"""
    return [sum(1 for i in row if i != o) for o, row in enumerate(_rows(m))]


def is_symmetric(m):
    """symmetric.rs:7-34; values compared with f64 `!=`"""
    shape, ip, ix, dt = m
    if shape[0] != shape[1]:
        return False
    rows = _rows(m)
    ip = np.asarray(ip).astype(np.int64)
    dt = np.asarray(dt, dtype=np.float64)
    for o, row in enumerate(rows):
        for k, i in enumerate(row):
            other = rows[i]
            if o not in other:                                   # get_outer_inner(inner_ind, outer_ind) is None
                return False
            if dt[ip[i] + other.index(o)] != dt[ip[o] + k]:
                return False
    return True


# ---- start strategies (ordering.rs:14-267) ---------------------------------------------------------------------------------------

def _first_unvisited(visited):
    return next(i for i, a in enumerate(visited) if not a)


def rls_contender_and_height(root, deg, rows):
    """ordering.rs:109-216"""
    visited = [False] * len(deg)
    visited[root] = True
    rls = [root]
    rls_index = 0
    height = 0
    current_level_countdown = 1
    next_level_countup = 0
    last_level_len = 1
    while rls_index < len(rls):
        parent = rls[rls_index]
        current_level_countdown -= 1
        for neighbor in rows[parent]:
            if not visited[neighbor]:
                visited[neighbor] = True
                next_level_countup += 1
                rls.append(neighbor)
        if current_level_countdown == 0:
            if next_level_countup > 0:
                last_level_len = next_level_countup
            current_level_countdown = next_level_countup
            next_level_countup = 0
            height += 1
        rls_index += 1
    last = rls[len(rls) - last_level_len:]
    contender = min(last, key=lambda i: deg[i])                  # min_by_key: the FIRST minimum
    return contender, height


def find_start_vertex(strategy, visited, deg, rows, trace=None):
    if strategy == NEXT:
        return _first_unvisited(visited)
    if strategy == MINIMUM_DEGREE:
        return min((i for i, a in enumerate(visited) if not a), key=lambda i: deg[i])
    current = _first_unvisited(visited)
    if deg[current] == 0:
        return current
    contender, current_height = rls_contender_and_height(current, deg, rows)
    swaps = 0
    while True:
        contender_contender, contender_height = rls_contender_and_height(contender, deg, rows)
        if contender_height > current_height:
            current_height = contender_height
            current = contender
            contender = contender_contender
            swaps += 1
        else:
            if trace is not None:
                trace.append(swaps)
            return current


# ---- cuthill_mckee_custom (ordering.rs:440-526) ----------------------------------------------------------------------------------

def _finish(n, order, parts, direction):
    if direction == FORWARD:
        return list(order), parts
    return list(reversed(order)), [n - p for p in reversed(parts)]


def cuthill_mckee(m, strategy=PSEUDO_PERIPHERAL, direction=REVERSED, trace=None):
    """-> (perm, connected_parts).  trace: a list that receives the swaps of every George-Liu loop."""
    shape = m[0]
    assert shape[0] == shape[1]
    rows = _rows(m)
    n = len(rows)
    deg = degrees(m)
    order, parts = [], []
    dq = deque()
    visited = [False] * n
    for perm_index in range(n):
        if dq:
            current = dq.popleft()
        else:
            parts.append(perm_index)
            current = find_start_vertex(strategy, visited, deg, rows, trace)
            if visited[current]:                                 # assert!(!visited[new_start_vertex]), ordering.rs:488-491
                raise StartVisited("Vertex returned by starting strategy should always be unvisited")
        order.append(current)
        visited[current] = True
        neighbors = []
        for nb in rows[current]:
            if not visited[nb]:
                neighbors.append((deg[nb], nb))
                visited[nb] = True
        neighbors.sort(key=lambda t: t[0])                       # stable
        for _, nb in neighbors:
            dq.append(nb)
    parts.append(n)
    return _finish(n, order, parts, direction)


def reverse_cuthill_mckee(m):
    return cuthill_mckee(m, PSEUDO_PERIPHERAL, REVERSED)


# ---- the level formulation: written independently of the loop above --------------------------------------------------------------

def _levels(root, rows, seen, key):
    """the levels from `root`; seen[v] is set for every vertex reached.  Level L + 1 = the unseen vertices adjacent to level L,
    each owned by its neighbour of smallest position, ordered by key(owner position, vertex)"""
    seen[root] = True
    out = [[root]]
    while True:
        owner = {}
        for pos, v in enumerate(out[-1]):
            for j in rows[v]:
                if j != v and not seen[j] and (j not in owner or pos < owner[j]):
                    owner[j] = pos
        if not owner:
            return out
        for j in owner:
            seen[j] = True
        out.append(sorted(owner, key=lambda j: key(owner[j], j)))


def cuthill_mckee_levels(m, strategy=PSEUDO_PERIPHERAL, direction=REVERSED):
    rows = _rows(m)
    n = len(rows)
    deg = degrees(m)
    by_degree = sorted(range(n), key=lambda v: (deg[v], v))
    seen = [False] * n
    order, parts = [], []

    def search(root):
        lv = _levels(root, rows, [False] * n, lambda pos, j: (pos, j))
        low = min(deg[v] for v in lv[-1])
        return next(v for v in lv[-1] if deg[v] == low), len(lv)

    while len(order) < n:
        parts.append(len(order))
        if strategy == MINIMUM_DEGREE:
            root = next(v for v in by_degree if not seen[v])
        else:
            root = next(v for v in range(n) if not seen[v])
            if strategy == PSEUDO_PERIPHERAL and deg[root]:
                contender, height = search(root)
                while True:
                    c2, h2 = search(contender)
                    if h2 <= height:
                        break
                    root, contender, height = contender, c2, h2
        if seen[root]:
            raise StartVisited("Vertex returned by starting strategy should always be unvisited")
        for level in _levels(root, rows, seen, lambda pos, j: (pos, deg[j], j)):
            order.extend(level)
    parts.append(n)
    return _finish(n, order, parts, direction)


# ---- helpers of the tests --------------------------------------------------------------------------------------------------------

def perm_inv(perm):
    inv = [0] * len(perm)
    for i, v in enumerate(perm):
        inv[v] = i
    return inv


def from_edges(n, edges, diag=True, symmetric=True):
    """(shape, indptr, indices, data) of the pattern with the given (i, j) pairs, mirrored when symmetric"""
    rows = [set() for _ in range(n)]
    for i, j in edges:
        rows[i].add(j)
        if symmetric:
            rows[j].add(i)
    if diag:
        for i in range(n):
            rows[i].add(i)
    ip = np.zeros(n + 1, dtype=np.int64)
    ix = []
    for r in range(n):
        ix.extend(sorted(rows[r]))
        ip[r + 1] = len(ix)
    ix = np.array(ix, dtype=np.int64)
    dt = np.ones(ix.size)
    return (n, n), ip, ix, dt


def random_pattern(n, seed, symmetric=True, density=None):
    rng = np.random.default_rng(seed)
    k = int(rng.integers(0, max(1, 2 * n))) if density is None else int(density * n)
    edges = [(int(rng.integers(0, n)), int(rng.integers(0, n))) for _ in range(k)]
    return from_edges(n, edges, diag=bool(rng.integers(0, 2)), symmetric=symmetric)


def bandwidth(m):
    rows = _rows(m)
    return max((abs(i - o) for o, r in enumerate(rows) for i in r), default=0)
