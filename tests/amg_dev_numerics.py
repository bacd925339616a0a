"""What the device-aggregation tests share, on top of amg_numerics, which is only read: the aggregation rule
restated in synchronous rounds, and the extra cases -- the priority path, the one-way pattern, the bound classes, the width
boundaries and the randomised sweep.  No GPU and no library call in here."""
import numpy as np

import amg_numerics as AN

# the rounds of the synchronous form on amg_numerics.CASES at seed 0, level 0, each case's own theta: what rounds_py below
# gives, pinned for sblas_amg_roots_rounds_ref (the device may take fewer, never more)
ROUNDS = {"n0": 0, "n1": 1, "diagonal300": 1, "tridiagonal3000": 6, "grid24": 6, "grid32": 7, "clique130": 6, "star5000": 3, "random4000": 9,
          "aniso32": 6}


def rounds_py(n, rp, ci, val=None, theta=0.0, seed=0, level=0):
    """The rule in synchronous rounds -> (root, rounds).  v is decided by the strong neighbours u of its own row with
    h(u) > h(v): a non-root as soon as one is a root, a root once all are non-roots; a round reads only the states of the
    rounds before it; rounds counts the rounds that decided a vertex."""
    strong = AN.strong_lists(n, rp, ci, val, theta)
    h = [AN.priority(v, seed, level) for v in range(n)]
    higher = [[u for u in strong[v] if h[u] > h[v]] for v in range(n)]
    state, rounds, waiting = [-1] * n, 0, list(range(n))
    while waiting:
        new = {}
        for v in waiting:
            if any(state[u] == 1 for u in higher[v]):
                new[v] = 0
            elif all(state[u] == 0 for u in higher[v]):
                new[v] = 1
        assert new, "the waiting vertex of greatest h waits for nobody"
        for v, s in new.items():
            state[v] = s
        waiting = [v for v in waiting if v not in new]
        rounds += 1
    return np.array([s == 1 for s in state], bool), rounds


def roots_are_numbered(root, agg, aggptr):
    """the roots of a set of aggregates carry the aggregates' numbers in ascending vertex order, one root an aggregate"""
    roots = np.flatnonzero(root)
    return len(roots) == len(aggptr) - 1 and np.array_equal(np.asarray(agg)[roots], np.arange(len(roots)))


def case_dict(name, n, rp, ci, val, theta=0.0):
    return dict(name=name, n=n, rp=rp, ci=ci, val=val, symmetric=False, theta=theta)


def priority_path(n=300, seed=0, level=0):
    """n vertices sorted by descending priority and joined in a path: each row is {previous, self, next}.  Vertex k of the
    order waits for vertex k - 1, so the synchronous form takes n rounds and every other vertex is a root."""
    order = sorted(range(n), key=lambda v: -AN.priority(v, seed, level))
    rows = [None] * n
    for k, v in enumerate(order):
        r = {v: 2.0}
        if k > 0:
            r[order[k - 1]] = -1.0
        if k + 1 < n:
            r[order[k + 1]] = -1.0
        rows[v] = r
    return case_dict("priority_path", *AN.csr_from_rows(rows))


def one_way(n=240, seed=0, level=0):
    """Row v names u while row u does not name v: v = 0 .. n/2 - 1 name three vertices of the upper half, which name nobody.
    -> (case, pairs): the one-way pairs (v, u), among which u has the higher h in some and the lower in others."""
    rng = np.random.default_rng(17)
    half = n // 2
    rows, pairs = [], []
    for v in range(n):
        r = {v: 4.0}
        if v < half:
            for u in rng.choice(np.arange(half, n), 3, replace=False):
                r[int(u)] = -1.0
                pairs.append((v, int(u)))
        rows.append(r)
    c = case_dict("one_way", *AN.csr_from_rows(rows))
    up = [AN.priority(u, seed, level) > AN.priority(v, seed, level) for v, u in pairs]
    assert any(up) and not all(up)
    for v, u in pairs:
        assert v not in c["ci"][c["rp"][u]:c["rp"][u + 1]].tolist()
    return c, pairs


BOUND_CLASSES = ("zeros", "nan", "inf", "equal")


def bound_class(kind, theta):
    """The 12 x 12 grid Laplacian with every fourth row's values replaced: `zeros` -- the only off-diagonals are +0.0 and
    -0.0 (bound 0: all strong); `nan` -- one NaN off-diagonal (never the maximum, never strong); `inf` -- one infinite
    one (bound theta * inf: only it is strong); `equal` -- equal magnitudes of both signs (all strong up to theta = 1)."""
    n, rp, ci, val = AN.csr_from_rows(AN.grid_rows(12))
    val = val.copy()
    for i in range(0, n, 4):
        off = [e for e in range(rp[i], rp[i + 1]) if ci[e] != i]
        if kind == "zeros":
            for k, e in enumerate(off):
                val[e] = 0.0 if k % 2 else -0.0
        elif kind == "nan":
            val[off[0]] = np.nan
        elif kind == "inf":
            val[off[-1]] = -np.inf if i % 8 else np.inf
        elif kind == "equal":
            for k, e in enumerate(off):
                val[e] = 0.75 if k % 2 else -0.75
        else:
            raise KeyError(kind)
    return case_dict("%s@%g" % (kind, theta), n, rp, ci, val, theta)


WIDTH_LENGTHS = (1, 2, 4, 5, 32, 33, 64, 65, 130)


def widths(theta=0.0):
    """400 rows whose stored lengths include both sides of every lane-group bound; columns drawn at random, the diagonal
    added; values (read when theta > 0) with exact zeros and ties"""
    rng = np.random.default_rng(400)
    n, rows = 400, []
    for i in range(n):
        length = WIDTH_LENGTHS[i % len(WIDTH_LENGTHS)] if i < 90 else int(rng.integers(1, 12))
        cols = {i}
        while len(cols) < length:
            cols.add(int(rng.integers(0, n)))
        r = {c: float(rng.choice([0.0, -0.5, 0.5, -1.0, 2.0, -0.25])) for c in cols}
        r[i] = 8.0
        rows.append(r)
    c = case_dict("widths@%g" % theta, *AN.csr_from_rows(rows), theta=theta)
    assert set(WIDTH_LENGTHS) <= set(np.diff(c["rp"]).tolist())
    return c


SWEEP = 24


def sweep_case(k):
    """pattern k of the randomised sweep: n from [1, 400], theta from {0, 0.25, 1}, from the fixed seed 2100 + k"""
    rng = np.random.default_rng(2100 + k)
    n = int(rng.integers(1, 401))
    theta = (0.0, 0.25, 1.0)[k % 3]
    most = int(rng.choice([3, 8, 40, 90]))
    rows = []
    for i in range(n):
        cols = set(int(c) for c in rng.integers(0, n, int(rng.integers(0, most + 1)))) | {i}
        r = {c: float(rng.choice([0.0, -1.0, 1.0, -0.5, 3.0])) * float(rng.integers(1, 3)) for c in cols}
        r[i] = 9.0
        rows.append(r)
    return case_dict("sweep%d" % k, *AN.csr_from_rows(rows), theta=theta)


def values(c):
    return c["val"] if c["theta"] > 0.0 else None
