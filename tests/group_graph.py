"""Synthetic graphs and plain references for the group-operator edge
tests (a helper module, not a test).

`group_graph()` is a second small deterministic graph, next to
`synth_graph.edge_graph()`, for the kernels the first one does not
reach: the OPTIONAL pair (`k_expand_opt`, `k_filter_opt`), the
predicate-variable kernel (`k_vu`) and the projection.  Its start types
have 1, 255, 256, 257, 513 and 1025 members, so the index start of a
plan puts a table on each side of the 256-row tile, and the degree of
the optional predicate is keyed on the member index, so every tile holds
rows with 0, 1, 2, 33 and 300 edges.  `group_graph(big=True)` adds one
start type of 2048 * 256 + 257 members for the second grid trip.

`single_typed_graph()` has no entity with two types, which is what the
light-query kernels (`k_light2`, `k_light_batch`) require of a store.

`optional_ref`, `vu_ref` and `light_ref` restate the operators over the
plain adjacency in numpy / Python and share no code with the engine or
the oracle.
"""
import numpy as np

from tests.synth_graph import B, IN, OUT, TYPE, adjacency

BLANK = 0xFFFFFFFF

# ---- group_graph ids --------------------------------------------------
P_OPT, P_OPT2, P_LIST, P_PAIR, P_TAG, P_NOSEG = 2, 3, 4, 5, 6, 7
MP_BASE = 10                       # many-predicate pids MP_BASE .. +129
MP_COUNTS = [1, 63, 64, 65, 130]   # distinct predicates per direction
GT_B, GT_O = 300, 301              # object types: the filter type / other
TG_A, TG_B, TG_C = 302, 303, 304   # small types of the tag vertices
START_SIZES = [1, 255, 256, 257, 513, 1025]
T_START = {n: 310 + k for k, n in enumerate(START_SIZES)}
T_NONE, T_ALL, T_BIG = 320, 321, 322
N_NONE = N_ALL = 257
N_BIG = 2048 * 256 + 257
# P_OPT degree of start member i is OPT_DEGS[i % 16]: each 256-row tile
# holds every class
OPT_DEGS = [2, 0, 1, 33, 300, 1, 0, 2, 33, 1, 0, 2, 1, 0, 1, 2]
N_OPOOL, N_ZPOOL = 600, 64

# ---- single_typed_graph ids -------------------------------------------
LT_F, LT_O = 20, 21                # the filter type / another type
P_L, P_X = 2, 3
LIGHT_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1000]
LOW_ID = 50                        # an id below the first vertex id

_NONE = np.empty(0, dtype=np.uint32)


class _Builder:
    def __init__(self):
        self.nxt = B
        self.trip = []

    def take(self, n):
        a = np.arange(self.nxt, self.nxt + n, dtype=np.uint32)
        self.nxt += n
        return a

    def add(self, s, p, o):
        s, o = np.broadcast_arrays(np.asarray(s, np.uint32),
                                   np.asarray(o, np.uint32))
        self.trip.append(np.stack([s.ravel(), np.full(s.size, p, np.uint32),
                                   o.ravel()], axis=1))

    def triples(self):
        return np.concatenate(self.trip).astype(np.uint32)


def opt_objects(opool, i, d):
    """The d P_OPT objects of start member i (distinct: d <= 300 < 600)."""
    return opool[(i * 7 + np.arange(d)) % N_OPOOL]


def group_graph(big=False):
    """(triples, meta).  Vertex ids of the small graph are the same with
    and without `big`; the big start type takes the ids after them."""
    g = _Builder()
    # P_OPT objects in three type classes by index: GT_B, GT_O, both
    opool = g.take(N_OPOOL)
    j = np.arange(N_OPOOL)
    g.add(opool[j % 3 != 1], TYPE, GT_B)
    g.add(opool[j % 3 != 0], TYPE, GT_O)
    # second optional predicate: object j has [0, 1, 2, 1][j % 4] edges
    zpool = g.take(N_ZPOOL)
    k = np.arange(N_ZPOOL)
    g.add(zpool[k % 2 == 0], TYPE, GT_B)
    g.add(zpool[k % 2 == 1], TYPE, GT_O)
    for jj in range(N_OPOOL):
        n2 = [0, 1, 2, 1][jj % 4]
        if n2:
            g.add(opool[jj], P_OPT2, zpool[(jj * 5 + np.arange(n2)) % N_ZPOOL])
    # tag vertices: single-typed, multi-typed, untyped (PK_INDEX group)
    tv = g.take(6)
    g.add(tv[[0, 1, 5]], TYPE, TG_A)
    g.add(tv[[1, 4]], TYPE, TG_B)
    g.add(tv[3], TYPE, TG_C)

    starts = {}

    def start_set(t, n, degs):
        subj = g.take(n)
        g.add(subj, TYPE, t)
        i = np.arange(n)
        g.add(subj, P_TAG, tv[i % 6])
        # P_PAIR: every second P_OPT object plus one vertex that is none
        g.add(subj, P_PAIR, zpool[i % N_ZPOOL])
        for ii in np.flatnonzero(degs):
            objs = opt_objects(opool, int(ii), int(degs[ii]))
            g.add(subj[ii], P_OPT, objs)
            g.add(subj[ii], P_PAIR, objs[::2])
        starts[t] = subj
        return subj

    for n in START_SIZES:
        start_set(T_START[n], n, np.resize(OPT_DEGS, n))
    start_set(T_NONE, N_NONE, np.zeros(N_NONE, dtype=int))
    start_set(T_ALL, N_ALL, 1 + np.arange(N_ALL) % 2)

    # constant with a P_LIST list over a third of every start set and
    # half of the P_OPT objects
    c_list = int(g.take(1)[0])
    for t, subj in starts.items():
        g.add(c_list, P_LIST, subj[::3])
    g.add(c_list, P_LIST, opool[::2])

    # many-predicate vertices: k distinct predicates in each direction,
    # 1..3 edges per predicate; mpool[2] is an object of the predicates
    # with j % 3 == 2 only
    mpool = g.take(8)
    mp = g.take(len(MP_COUNTS))
    for m, cnt in zip(mp, MP_COUNTS):
        for jj in range(cnt):
            g.add(m, MP_BASE + jj, mpool[:1 + jj % 3])
            g.add(mpool[3:4 + jj % 3], MP_BASE + jj, m)
    # predicates (and a type) in the OUT direction, none in the IN one
    oneway = int(g.take(1)[0])
    g.add(oneway, MP_BASE, mpool[0])
    g.add(oneway, MP_BASE + 1, mpool[:2])
    g.add(oneway, MP_BASE + 2, mpool[1])
    g.add(oneway, TYPE, GT_O)
    absent = int(g.take(1)[0])          # in range, no triple at all
    last = int(g.take(1)[0])
    g.add(last, P_TAG, tv[0])

    meta = dict(opool=opool, zpool=zpool, tv=tv, starts=starts, c_list=c_list,
                mpool=mpool, mp=mp, oneway=oneway, absent=absent,
                sub_base=[5, B - 1])
    if big:
        subj = g.take(N_BIG)
        g.add(subj, TYPE, T_BIG)
        odd = np.arange(1, N_BIG, 2)
        g.add(subj[odd], P_OPT, opool[odd % N_OPOOL])
        starts[T_BIG] = subj
    triples = g.triples()
    meta["max_id"] = int(triples[:, [0, 2]].max())
    meta["past_max"] = meta["max_id"] + 1
    return triples, meta


def single_typed_graph():
    """(triples, meta): no entity has two types.  Constants with P_L
    lists of LIGHT_SIZES entries over a pool typed LT_F / LT_O / untyped
    by index; three lists also hold LOW_ID and/or the last vid."""
    g = _Builder()
    lpool = g.take(1200)
    k = np.arange(1200)
    g.add(lpool[k % 3 == 0], TYPE, LT_F)
    g.add(lpool[k % 3 == 1], TYPE, LT_O)
    consts = g.take(len(LIGHT_SIZES))
    absent = int(g.take(1)[0])
    last = int(g.take(1)[0])
    g.add(last, TYPE, LT_F)
    g.add(consts, P_X, lpool[0])        # every constant is in the graph
    # (size, holds LOW_ID, holds the last vid)
    extra = {65: (True, True), 257: (False, True), 1000: (True, True)}
    for idx, (c, n) in enumerate(zip(consts, LIGHT_SIZES)):
        low, lst = extra.get(n, (False, False))
        m = n - int(low) - int(lst)
        g.add(c, P_L, lpool[11 * idx:11 * idx + m])
        if low:
            g.add(c, P_L, LOW_ID)
        if lst:
            g.add(c, P_L, last)
    triples = g.triples()
    meta = dict(lpool=lpool, consts=consts, absent=absent, last=last,
                max_id=int(triples[:, [0, 2]].max()))
    return triples, meta


def group_adjacency(triples):
    """synth_graph.adjacency plus the type index lists, which the
    per-row `?t rdf:type-IN ?x` expansion reads: (t, TYPE, IN) -> the
    sorted members of type t."""
    adj = adjacency(triples)
    tt = triples[triples[:, 1] == TYPE]
    for t in np.unique(tt[:, 2]).tolist():
        adj[(t, TYPE, IN)] = np.unique(tt[tt[:, 2] == t, 0]).astype(np.uint32)
    return adj


def pred_lists(adj):
    """{(vid, dir): ascending predicate ids}: the adjacency grouped by
    predicate.  rdf:type counts as an OUT predicate of a typed vertex;
    the type index lists are no predicate of the type id."""
    out = {}
    for (v, p, d) in adj:
        if p == TYPE and d == IN:
            continue
        out.setdefault((v, d), []).append(p)
    return {k: sorted(v) for k, v in out.items()}


def _member_mask(vals, tgts, adj, p, d):
    """ok[r]: tgts[r] is a (p, d) neighbour of vals[r]; BLANK on either
    side never is."""
    uniq, inv = np.unique(vals, return_inverse=True)
    inv = inv.ravel()
    lists = [_NONE if int(u) == BLANK else adj.get((int(u), p, d), _NONE)
             for u in uniq]
    if np.isscalar(tgts):
        ok_u = np.array([bool(np.isin(tgts, x)) for x in lists], dtype=bool)
        return ok_u[inv] if len(inv) else np.zeros(0, dtype=bool)
    sets = [set(x.tolist()) for x in lists]
    return np.array([t != BLANK and t in sets[j]
                     for t, j in zip(tgts.tolist(), inv.tolist())], dtype=bool)


def optional_ref(base_rows, group_patterns, adj):
    """The OPTIONAL group over a base table whose column k holds variable
    -(k + 1); a variable first bound inside the group takes the next
    column.  Patterns are Plan tuples (s, p, dir, o).

    Rows are never dropped and every row carries a matched flag that
    starts set.  An expansion (`?known p ?new`) emits one row per
    neighbour; a row whose flag is clear, whose start is BLANK or that
    has no neighbour stays as one row with BLANK in the new column, its
    flag unchanged.  A filter (`?known p ?known`, `?known p const`,
    `const p ?known`) that fails writes BLANK into every column first
    bound inside the group, if the flag was still set, and clears the
    flag."""
    tbl = np.array(base_rows, dtype=np.uint32)
    tbl = tbl.reshape(len(tbl), -1)
    v2c = {-(c + 1): c for c in range(tbl.shape[1])}
    flag = np.ones(len(tbl), dtype=bool)
    born = []
    for s, p, d, o in group_patterns:
        if s < 0 and o < 0 and o not in v2c:
            vals = tbl[:, v2c[s]]
            uniq, inv = np.unique(vals, return_inverse=True)
            inv = inv.ravel()
            lists = [_NONE if int(u) == BLANK
                     else adj.get((int(u), p, d), _NONE) for u in uniq]
            deg = np.array([len(x) for x in lists], dtype=np.int64)[inv] \
                if len(inv) else np.zeros(0, dtype=np.int64)
            deg[~flag] = 0
            cnt = np.maximum(deg, 1)
            first = np.cumsum(cnt) - cnt
            new = np.full(int(cnt.sum()), BLANK, dtype=np.uint32)
            live = np.flatnonzero(deg)
            if len(live):
                dl = deg[live]
                within = np.arange(int(dl.sum())) - np.repeat(
                    np.cumsum(dl) - dl, dl)
                new[np.repeat(first[live], dl) + within] = np.concatenate(
                    [lists[jx] for jx in inv[live].tolist()])
            tbl = np.column_stack([np.repeat(tbl, cnt, axis=0), new])
            flag = np.repeat(flag, cnt)
            v2c[o] = tbl.shape[1] - 1
            born.append(v2c[o])
            continue
        if s >= 0:
            ok = np.isin(tbl[:, v2c[o]], adj.get((s, p, d), _NONE))
        else:
            tgt = int(o) if o >= 0 else tbl[:, v2c[o]]
            ok = _member_mask(tbl[:, v2c[s]], tgt, adj, p, d)
        wipe = flag & ~ok
        for c in born:
            tbl[wipe, c] = BLANK
        flag = flag & ok
    return tbl


def vu_ref(table, col, adj, plists, d, const=None, start=None):
    """One predicate-variable step.  Every input row (or the constant
    `start`, a table of one empty row) is extended, per predicate p of
    its start vertex in ascending order, by (p, y) for each (p, d)
    neighbour y — or, with `const`, by (p) alone when `const` is one."""
    if start is not None:
        rows, keys = [[]], [int(start)]
    else:
        rows = np.asarray(table, dtype=np.uint32).tolist()
        keys = [r[col] for r in rows]
    width = (len(rows[0]) if rows else np.asarray(table).shape[1]) + \
        (1 if const is not None else 2)
    memo, out = {}, []
    for row, v in zip(rows, keys):
        if v not in memo:
            ext = []
            for p in plists.get((v, d), ()):
                lst = adj[(v, p, d)].tolist()
                if const is None:
                    ext += [[p, y] for y in lst]
                elif const in lst:
                    ext.append([p])
            memo[v] = ext
        out += [row + e for e in memo[v]]
    return np.array(out, dtype=np.uint32).reshape(len(out), width)


def light_ref(adj, const, pid, d, cval):
    """`const pid ?x . ?x rdf:type cval` on a single-typed graph: the
    list members whose one type is cval, in list order."""
    lst = adj.get((int(const), pid, d), _NONE)
    keep = [v for v in lst.tolist()
            if cval in adj.get((v, TYPE, OUT), _NONE).tolist()]
    return np.array(keep, dtype=np.uint32)
