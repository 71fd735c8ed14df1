"""Edge tests for the kernels outside the plain-BGP operators: the
OPTIONAL pair (k_expand_opt / k_filter_opt), the predicate-variable
kernel (k_vu), the fork-join split (k_dst_count / scan2 / scatter2),
the single-block peer step (k_peer_step), the light-query kernels
(k_light2 / k_light_batch) and the device projection (k_project).

The inputs come from group_graph.py (and, for the peer step, the graph
of synth_graph.py): start sets and tables on the 256-row tile, a second
grid trip, vertices with more predicates than a wavefront has lanes,
split destinations from 1 to 64, a store without multi-typed entities.

CPU part (unmarked): the graphs have the designed properties and every
plain reference (optional_ref, vu_ref, light_ref, step_ref) equals the
oracle on every case.  GPU part: the engine against those references
only, exactly.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import wukong_amd as wk
from wukong_amd import Plan
from tests import filter_ref
from tests import group_graph as gg
from tests import synth_graph as sg
from tests import test_gpu_operator_edges as T
from tests.group_graph import (BLANK, GT_B, GT_O, MP_BASE, MP_COUNTS, P_LIST,
                               P_OPT, P_OPT2, P_PAIR, P_TAG, START_SIZES,
                               T_ALL, T_BIG, T_NONE, T_START, LT_F, LT_O, P_L,
                               optional_ref, vu_ref, light_ref)
from tests.oracle_util import OracleCtx, OracleExecutor, sort_rows
from tests.synth_graph import B, IN, OUT, TYPE, env, step_ref

ROWS = T.ROWS
X, Y, Z, W = -1, -2, -3, -4
STORE_ENVS = {"default": {}, "hash": dict(WK_FN=0, WK_CSR=0, WK_TBM=0)}
SETS = [T_START[n] for n in START_SIZES] + [T_NONE, T_ALL]
VU_BIG = 4096 + 257          # second trip of k_vu's 4096-block grid
SPLIT_BIG = 1024 * 256 + 257  # several 256-row trips per block of 1024
PEER_ROWS = [0, 1, 255, 256, 257, 511, 512, 513, 1025]
NDST = [1, 2, 3, 7, 8, 63, 64]


def _eq(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(sort_rows(got), want), what


class GCtx:
    """One graph, its plain adjacency, the oracle, and the references
    computed once per case."""

    def __init__(self, triples, meta):
        self.triples, self.meta = triples, meta
        self.adj = gg.group_adjacency(triples)
        self.plists = gg.pred_lists(self.adj)
        self.ora = OracleCtx(triples)
        self._ref = {}

    def members(self, t):
        return self.adj[(t, TYPE, IN)]

    def memo(self, key, fn):
        if key not in self._ref:
            r = sort_rows(fn())
            r.setflags(write=False)
            self._ref[key] = r
        return self._ref[key]

    def opt_want(self, group, t):
        return self.memo(("opt", group, t), lambda: optional_ref(
            self.members(t)[:, None], groups(self.meta)[group], self.adj))


@pytest.fixture(scope="module")
def gctx():
    return GCtx(*gg.group_graph())


@pytest.fixture(scope="module")
def bigctx():
    """The graph with the 2048 * 256 + 257 member start type: only the
    two second-grid-trip tests pay for it."""
    return GCtx(*gg.group_graph(big=True))


@pytest.fixture(scope="module")
def lctx():
    return GCtx(*gg.single_typed_graph())


@pytest.fixture(scope="module")
def ectx():
    return T.Ctx()


# ---------------------------------------------------------------------
# OPTIONAL cases
# ---------------------------------------------------------------------
def groups(meta):
    c = int(meta["c_list"])
    return {
        "k2u": [(X, P_OPT, OUT, Y)],
        "k2u-type": [(X, P_OPT, OUT, Y), (Y, TYPE, OUT, GT_B)],
        # 3 patterns; the filter on ?z blanks two columns
        "k2u-k2u-type": [(X, P_OPT, OUT, Y), (Y, P_OPT2, OUT, Z),
                         (Z, TYPE, OUT, GT_B)],
        # the expansion after the filter reads cleared flags
        "k2u-type-k2u": [(X, P_OPT, OUT, Y), (Y, TYPE, OUT, GT_B),
                         (Y, P_OPT2, OUT, Z)],
        "c2k": [(X, P_OPT, OUT, Y), (c, P_LIST, OUT, Y)],      # PM_LIST
        "c2k-k2u": [(c, P_LIST, OUT, X), (X, P_OPT, OUT, Y)],
        "k2k": [(X, P_OPT, OUT, Y), (X, P_PAIR, OUT, Y)],      # PM_COL
        # ?x -> tag vertex -> its types (0, 1 or 2) -> their members:
        # three expansions, the last one keyed by type id (PK_INDEX),
        # with a BLANK start where the tag vertex is untyped
        "index": [(X, P_TAG, OUT, Y), (Y, TYPE, OUT, Z), (Z, TYPE, IN, W)],
    }


GROUPS = list(groups(dict(c_list=0)))
FILTERING = [g for g in GROUPS if g not in ("k2u", "index")]


def opt_plan(meta, group, t):
    pats = groups(meta)[group]
    nv = -min(min(s, o) for s, p, d, o in pats)
    return Plan([(t, TYPE, IN, X)], nv, [-(k + 1) for k in range(nv)],
                optional=pats)


def union_opt_plan():
    t = T_START[257]
    return Plan([(t, TYPE, IN, X)], 3, [X, Y, Z],
                unions=[[(X, P_TAG, OUT, Y)], [(X, P_PAIR, OUT, Y)]],
                optional=[(Y, P_OPT2, OUT, Z)])


def union_opt_want(cx):
    def fn():
        base = cx.members(T_START[257])[:, None]
        u = np.vstack([step_ref(base, 0, cx.adj, "k2u", P_TAG, OUT),
                       step_ref(base, 0, cx.adj, "k2u", P_PAIR, OUT)])
        return optional_ref(u, [(Y, P_OPT2, OUT, Z)], cx.adj)
    return cx.memo("union-opt", fn)


FILTERS = {"bound": ("bound", Y), "not-bound": ("not", ("bound", Y))}


def filter_plan(name):
    return Plan([(T_START[513], TYPE, IN, X)], 2, [X, Y],
                optional=[(X, P_OPT, OUT, Y)], filters=[FILTERS[name]])


def filter_want(cx, name):
    def fn():
        full = np.array(cx.opt_want("k2u", T_START[513]))
        keep = full[:, 1] != BLANK
        return full[keep if name == "bound" else ~keep]
    return cx.memo(("filter", name), fn)


# ---------------------------------------------------------------------
# VERSATILE cases
# ---------------------------------------------------------------------
VU_MODES = [(OUT, "new"), (IN, "new"), (OUT, "const"), (IN, "const")]


def vu_start_values(meta):
    s = meta["starts"]
    vals = list(meta["mp"]) + [meta["oneway"]] + list(meta["mpool"]) + \
        [s[T_START[257]][4], s[T_START[257]][1], meta["opool"][0],
         meta["opool"][2], meta["tv"][1], meta["absent"]] + \
        meta["sub_base"] + [meta["max_id"], meta["past_max"]]
    return np.array(vals, dtype=np.uint32)


def vu_const(meta, d):
    # mpool[2] is an object of the predicates MP_BASE + j with
    # j % 3 == 2 only; mpool[4] a subject of those with j % 3 >= 1
    return int(meta["mpool"][2] if d == OUT else meta["mpool"][4])


class VuCase:
    def __init__(self, cx, d, mode, n, ncols, col):
        self.d, self.mode, self.n, self.ncols, self.col = d, mode, n, ncols, col
        self.id = "vu-%s-%s-n%d-c%d" % ("out" if d == OUT else "in", mode, n,
                                        ncols)
        vals = vu_start_values(cx.meta)
        r = np.arange(n, dtype=np.int64)
        t = np.empty((n, ncols), dtype=np.uint32)
        for j in range(ncols):
            t[:, j] = B + (r * (j + 3) + j) % 1000
        t[:, col] = np.resize(vals, n) if n else vals[:0]
        self.table = t
        self.const = vu_const(cx.meta, d) if mode == "const" else None
        extra = 1 if mode == "const" else 2
        o = self.const if mode == "const" else -(ncols + 2)
        self.plan = Plan([(-(col + 1), -(ncols + 1), d, o)],
                         nvars=ncols + extra, required_vars=[-1])
        self.v2c = list(range(ncols)) + [-1] * extra
        self._cx = cx

    def ref(self):
        cx = self._cx
        return cx.memo(self.id, lambda: vu_ref(
            self.table, self.col, cx.adj, cx.plists, self.d, const=self.const))


_VU = {}


def vu_cases(cx, d, mode):
    """ROWS and the second grid trip, widths cycling; every width at one
    odd row count.  A table has at most 8 columns, so the two appended
    columns of the (p, y) mode leave room for 6, not 7."""
    key = (id(cx), d, mode)
    if key not in _VU:
        widths = [1, 2, 4, 7] if mode == "const" else [1, 2, 4, 6]
        cases = []
        for i, n in enumerate(ROWS + [VU_BIG]):
            c = widths[i % 4]
            cases.append(VuCase(cx, d, mode, n, c, i % c))
        have = {(k.n, k.ncols) for k in cases}
        for c in widths:
            if (257, c) not in have:
                cases.append(VuCase(cx, d, mode, 257, c, c - 1))
        _VU[key] = cases
    return _VU[key]


def vu_plans(meta):
    """Whole plans: name -> (plan, reference arguments)."""
    t = T_START[257]
    m = int(meta["mp"][4])
    out = {}
    for d, dn in ((OUT, "out"), (IN, "in")):
        out["k2uu-" + dn] = Plan([(t, TYPE, IN, X), (X, Y, d, Z)], 3,
                                 [X, Y, Z])
        # const start: the first pattern, one block
        out["c2uu-" + dn] = Plan([(m, X, d, Y)], 2, [X, Y])
        out["c2uc-" + dn] = Plan([(m, X, d, vu_const(meta, d))], 1, [X])
    return out


def vu_plan_want(cx, name):
    def fn():
        d = OUT if name.endswith("out") else IN
        m = int(cx.meta["mp"][4])
        if name.startswith("k2uu"):
            return vu_ref(cx.members(T_START[257])[:, None], 0, cx.adj,
                          cx.plists, d)
        const = vu_const(cx.meta, d) if name.startswith("c2uc") else None
        return vu_ref(None, 0, cx.adj, cx.plists, d, const=const, start=m)
    return cx.memo(("vu-plan", name), fn)


# ---------------------------------------------------------------------
# split, peer-step, light and projection inputs
# ---------------------------------------------------------------------
def split_table(n, ncols, col, ndst, pattern):
    r = np.arange(n, dtype=np.int64)
    t = np.empty((n, ncols), dtype=np.uint32)
    for j in range(ncols):
        t[:, j] = B + (r * (j + 5) + 3 * j) % 4099
    if pattern == "uniform":
        v = B + (r * 2654435761 + 12345) % 1000003
    elif pattern == "one":          # every row to one destination
        v = (B + r) // ndst * ndst + ndst // 2
    else:                           # only destinations ndst - 1 and 0
        v = (B + r) // ndst * ndst + np.where(r % 4 == 3, 0, ndst - 1)
    t[:, col] = v
    return t


def split_cases(ndst):
    """(rows, ncols, split column, pattern): ROWS with widths and value
    patterns cycling, and every split column of every width at 257."""
    pats = ["uniform", "one", "ends"]
    out = []
    for i, n in enumerate(ROWS):
        c = T.NCOLS[i % 4]
        for k, pat in enumerate(pats):
            out.append((n, c, (i + k) % c, pat))
    for c in T.NCOLS:
        for col in range(c):
            out.append((257, c, col, pats[(c + col) % 3]))
    return out


def split_plan(ncols, col):
    return Plan([(-(col + 1), P_OPT, OUT, -(ncols + 1))], nvars=ncols + 1,
                required_vars=[-1])


_PEER = {}


def peer_cases(cx, op):
    if op not in _PEER:
        widths = [c for c in T.NCOLS if c >= (2 if T.OPS[op][0] == "k2k" else 1)]
        cases = []
        for i, n in enumerate(PEER_ROWS):
            c = widths[i % len(widths)]
            cases.append(T.StepCase(cx, op, n, c, i % c))
        have = {(k.n, k.ncols) for k in cases}
        for c in widths:
            if (257, c) not in have:
                cases.append(T.StepCase(cx, op, 257, c, c - 1))
        _PEER[op] = cases
    return _PEER[op]


def light_plan(const, cval=LT_F):
    return Plan([(int(const), P_L, OUT, X), (X, TYPE, OUT, cval)], nvars=1,
                required_vars=[X])


def proj_cases(ncols):
    """name -> required_vars over a table of `ncols` columns plus one
    variable without a column."""
    ident = [-(k + 1) for k in range(ncols)]
    unb = -(ncols + 1)
    cyc = (ident + [unb]) * 9
    return {
        "identity": ident,
        "reversed": ident[::-1],
        "subset": ident[::2] if ncols > 1 else ident,
        "unbound": ident[:1] + [unb] + ident[1:],
        "repeat8": cyc[:8],      # device path
        "repeat9": cyc[:9],      # host path
        "repeat-one": [ident[-1]] * 8,
    }


def proj_table(ncols):
    r = np.arange(257, dtype=np.int64)
    return np.stack([(B + r * (j + 2) + 7 * j).astype(np.uint32)
                     for j in range(ncols)], axis=1)


def proj_want(table, req):
    cols = [table[:, -(v + 1)] if -(v + 1) < table.shape[1]
            else np.full(len(table), BLANK, dtype=np.uint32) for v in req]
    return np.stack(cols, axis=1)


# ---------------------------------------------------------------------
# CPU part
# ---------------------------------------------------------------------
def test_edge_graph_unchanged():
    """edge_graph() is pinned by the first suite: same triples, same last
    vid as before this module existed."""
    triples, meta = sg.edge_graph()
    assert triples.shape == (64030, 3) and meta["max_id"] == 149542


def test_group_graph_invariants(gctx):
    meta, adj = gctx.meta, gctx.adj
    assert len(gctx.triples) < 110000
    store = wk.Store(gctx.triples)
    assert store.check() == 0
    for n in START_SIZES:
        assert len(gctx.members(T_START[n])) == n
    # every 256-row tile of every start set holds all degree classes
    for t in SETS[1:6]:
        m = gctx.members(t)
        deg = np.array([len(adj.get((int(v), P_OPT, OUT), ())) for v in m])
        for lo in range(0, len(m) - 15, 256):
            assert set(deg[lo:lo + 256]) >= {0, 1, 2, 33, 300} or \
                len(m) - lo < 16, (t, lo)
        assert np.array_equal(store.get_index(t, IN), m)
    assert all((int(v), P_OPT, OUT) not in adj for v in gctx.members(T_NONE))
    assert all((int(v), P_OPT, OUT) in adj for v in gctx.members(T_ALL))
    # three type classes among the P_OPT objects
    kinds = {tuple(adj[(int(o), TYPE, OUT)].tolist()) for o in meta["opool"]}
    assert kinds == {(GT_B,), (GT_O,), (GT_B, GT_O)}
    # P_OPT objects with and without a P_OPT2 edge
    n2 = [len(adj.get((int(o), P_OPT2, OUT), ())) for o in meta["opool"]]
    assert set(n2) == {0, 1, 2}
    # many-predicate vertices, both directions; the one-way vertex
    for m, cnt in zip(meta["mp"], MP_COUNTS):
        for d in (OUT, IN):
            want = list(range(MP_BASE, MP_BASE + cnt))
            assert gctx.plists[(int(m), d)] == want
            assert list(store.get_triples(int(m), 0, d)) == want
            assert list(gctx.ora.get_triples(int(m), 0, d)) == want
    ow = meta["oneway"]
    assert gctx.plists[(ow, OUT)] == [TYPE, MP_BASE, MP_BASE + 1, MP_BASE + 2]
    assert (ow, IN) not in gctx.plists
    assert len(store.get_triples(ow, 0, IN)) == 0
    # the const ends are in some predicates' lists and not in others
    for d in (OUT, IN):
        c = vu_const(meta, d)
        hit = [c in adj[(int(meta["mp"][4]), p, d)].tolist()
               for p in gctx.plists[(int(meta["mp"][4]), d)]]
        assert any(hit) and not all(hit)
    # the PM_LIST constant covers part of every start set
    lst = adj[(meta["c_list"], P_LIST, OUT)]
    for t in SETS[1:]:
        k = np.isin(gctx.members(t), lst).sum()
        assert 0 < k < len(gctx.members(t))
    assert (meta["absent"], OUT) not in gctx.plists
    assert meta["absent"] < meta["max_id"]


@pytest.mark.parametrize("group", GROUPS)
def test_optional_ref_vs_oracle(gctx, group):
    for t in SETS:
        want = gctx.opt_want(group, t)
        got = gctx.ora.run_query(opt_plan(gctx.meta, group, t))
        _eq(got, want, (group, t))
        n = len(gctx.members(t))
        assert len(want) >= n                       # rows are never dropped
        if n >= 255 and t not in (T_NONE, T_ALL):
            # not vacuous: matched and BLANK rows both occur
            assert (want[:, -1] == BLANK).any(), (group, t)
            assert (want[:, -1] != BLANK).any(), (group, t)
        if n >= 255 and t != T_NONE and group in FILTERING:
            # the filter blanked some expanded rows and kept others
            full = gctx.opt_want("k2u", t)
            ycol = 1
            assert (full[:, ycol] != BLANK).sum() > \
                (want[:, ycol] != BLANK).sum() > 0, (group, t)
    # the all-BLANK and the all-matched set
    if group != "index":
        assert (gctx.opt_want(group, T_NONE)[:, 1] == BLANK).all()
    if group == "k2u":
        assert (gctx.opt_want(group, T_ALL)[:, 1] != BLANK).all()


def test_optional_k2u_vs_brute_left_join(gctx):
    """The one-pattern group is a plain left join: dict restatement."""
    out = {}
    for s, p, o in gctx.triples.tolist():
        if p == P_OPT:
            out.setdefault(s, []).append(o)
    for t in SETS:
        rows = []
        for v in gctx.members(t).tolist():
            rows += [[v, o] for o in out.get(v, [BLANK])]
        _eq(np.array(rows, dtype=np.uint32), gctx.opt_want("k2u", t), t)


def test_optional_big_ref_vs_oracle(bigctx):
    assert len(bigctx.members(T_BIG)) == gg.N_BIG == 2048 * 256 + 257
    for group in ("k2u", "k2u-type"):
        want = bigctx.opt_want(group, T_BIG)
        got = bigctx.ora.run_query(opt_plan(bigctx.meta, group, T_BIG))
        _eq(got, want, group)
        assert len(want) == gg.N_BIG
        assert 0 < (want[:, 1] != BLANK).sum() < gg.N_BIG
    assert (bigctx.opt_want("k2u-type", T_BIG)[:, 1] != BLANK).sum() < \
        (bigctx.opt_want("k2u", T_BIG)[:, 1] != BLANK).sum()


def test_union_filter_refs_vs_oracle(gctx):
    want = union_opt_want(gctx)
    _eq(gctx.ora.run_query(union_opt_plan()), want, "union-opt")
    assert (want[:, 2] == BLANK).any() and (want[:, 2] != BLANK).any()
    full = gctx.opt_want("k2u", T_START[513])
    for name in FILTERS:
        want = filter_want(gctx, name)
        _eq(filter_ref.expected(gctx.ora, filter_plan(name)), want, name)
        assert 0 < len(want) < len(full), name


@pytest.mark.parametrize("d,mode", VU_MODES)
def test_vu_ref_vs_oracle(gctx, d, mode):
    for case in vu_cases(gctx, d, mode):
        ex = OracleExecutor(gctx.ora, case.plan)
        ex.load(case.table, case.v2c, 0)
        ex.step()
        want = case.ref()
        _eq(ex.table(), want, case.id)
        if case.n >= 255:
            assert len(want) > 0, case.id
    # the const end keeps fewer rows than the (p, y) mode emits
    if mode == "const":
        a = vu_cases(gctx, d, "const")[7]
        b = vu_cases(gctx, d, "new")[7]
        assert a.n == b.n == 257 and 0 < len(a.ref()) < len(b.ref())


def test_vu_plans_ref_vs_oracle(gctx):
    for name, plan in vu_plans(gctx.meta).items():
        want = vu_plan_want(gctx, name)
        _eq(gctx.ora.run_query(plan), want, name)
        _eq(gctx.ora.brute_query(plan), want, (name, "brute"))
        assert len(want) > 0, name
    m = int(gctx.meta["mp"][4])
    assert len(vu_plan_want(gctx, "c2uu-out")) == sum(
        1 + j % 3 for j in range(130))
    assert len(vu_plan_want(gctx, "c2uc-out")) == len(range(2, 130, 3))
    assert gctx.plists[(m, OUT)][-1] == MP_BASE + 129


def test_split_inputs():
    """Each value pattern sends rows where it says."""
    for ndst in NDST:
        for pat, want in (("one", {ndst // 2}), ("ends", {0, ndst - 1})):
            t = split_table(1025, 2, 1, ndst, pat)
            assert set((t[:, 1] % ndst).tolist()) == want
        t = split_table(2049, 2, 1, ndst, "uniform")
        assert len(set((t[:, 1] % ndst).tolist())) == ndst


@pytest.mark.parametrize("op", list(T.OPS))
def test_peer_cases_step_ref_vs_oracle(ectx, op):
    for case in peer_cases(ectx, op):
        ex = OracleExecutor(ectx.ora, case.plan)
        ex.load(case.table, case.v2c, 0)
        ex.step()
        want = case.ref()
        _eq(ex.table(), want, case.id)
        if case.n >= 255 and op != "k2c-rfn-none":
            assert 0 < len(want), case.id
        if case.mode != "k2u" and case.n >= 255:
            assert len(want) < case.n, case.id


def test_single_typed_graph_and_light_ref(lctx):
    meta, adj = lctx.meta, lctx.adj
    store = wk.Store(lctx.triples)
    assert store.check() == 0
    tt = lctx.triples[lctx.triples[:, 1] == TYPE]
    subj, cnt = np.unique(tt[:, 0], return_counts=True)
    assert cnt.max() == 1                      # single-typed
    sizes = [len(adj.get((int(c), P_L, OUT), ())) for c in meta["consts"]]
    assert sizes == gg.LIGHT_SIZES
    for c, n in zip(meta["consts"], sizes):
        assert len(store.get_triples(int(c), P_L, OUT)) == n
    big = adj[(int(meta["consts"][-1]), P_L, OUT)]
    assert big[0] == gg.LOW_ID < B and big[-1] == meta["last"] == meta["max_id"]
    for c in list(meta["consts"]) + [meta["absent"]]:
        for cval in (LT_F, LT_O):
            want = light_ref(adj, c, P_L, OUT, cval)
            got = lctx.ora.run_query(light_plan(c, cval))
            _eq(got, sort_rows(want[:, None]), (int(c), cval))
            _eq(lctx.ora.brute_query(light_plan(c, cval)),
                sort_rows(want[:, None]), (int(c), cval, "brute"))
    for c, n in zip(meta["consts"], sizes):
        if n >= 63:                            # a keyed mix: strict subset
            assert 0 < len(light_ref(adj, c, P_L, OUT, LT_F)) < n
    # the last vid passes the filter, the low id never does
    assert meta["last"] in light_ref(adj, meta["consts"][-1], P_L, OUT, LT_F)
    assert gg.LOW_ID not in light_ref(adj, meta["consts"][-1], P_L, OUT, LT_F)


def test_projection_reference():
    t = proj_table(4)
    for name, req in proj_cases(4).items():
        want = proj_want(t, req)
        assert want.shape == (257, len(req))
        for j, v in enumerate(req):
            col = want[:, j]
            assert (col == BLANK).all() if v == -5 else \
                np.array_equal(col, t[:, -(v + 1)]), name


# ---------------------------------------------------------------------
# GPU part
# ---------------------------------------------------------------------
# engines count their launches per category (kernel_stats), which is how
# the tests see that the kernel under test ran
TIMED = dict(WK_KERNEL_TIMING=1)


def _engines(triples):
    out = {}
    for name, kv in STORE_ENVS.items():
        with env(**kv, **TIMED):
            out[name] = wk.Engine(wk.Store(triples), device=0)
    return out


@pytest.fixture(scope="module")
def engines(gctx):
    return _engines(gctx.triples)


def _launches(eng):
    return {k: v["launches"] for k, v in eng.kernel_stats().items()}


def _delta(eng, before):
    now = _launches(eng)
    return {k: now[k] - before[k] for k in now}


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("config", list(STORE_ENVS))
def test_optional_groups(gctx, engines, config, group):
    """`<T> rdf:type-IN ?x` + one OPTIONAL group over every start-set
    size, the all-BLANK and the all-matched set: k_expand_opt's per-tile
    append base at 255/256/257/513/1025 rows, BLANK and flag-clear
    starts, PM_CONST / PM_LIST / PM_COL in k_filter_opt, the PK_INDEX
    expansion, a blank mask of two bits and three flag swaps."""
    eng = engines[config]
    for t in SETS:
        before = _launches(eng)
        got = eng.run_query(opt_plan(gctx.meta, group, t))
        _eq(got, gctx.opt_want(group, t), (group, t))
        d = _delta(eng, before)
        # the group's expansions are the plan's only expand launches,
        # its filters the only filter launches
        pats = groups(gctx.meta)[group]
        nexp = sum(1 for s, p, dd, o in pats if s < 0 and o < 0
                   and not (group == "k2k" and p == P_PAIR))
        assert d["expand"] == nexp and d["filter"] == len(pats) - nexp, \
            (group, t, d)


@pytest.mark.gpu
def test_optional_second_grid_trip(bigctx):
    """2048 * 256 + 257 start rows: every block of the OPTIONAL kernels
    takes a second trip of its grid-stride loop, the last one partial."""
    for name, eng in _engines(bigctx.triples).items():
        for group in ("k2u", "k2u-type"):
            got = eng.run_query(opt_plan(bigctx.meta, group, T_BIG))
            _eq(got, bigctx.opt_want(group, T_BIG), (name, group))


@pytest.mark.gpu
def test_union_then_optional_and_filter(gctx, engines):
    for name, eng in engines.items():
        _eq(eng.run_query(union_opt_plan()), union_opt_want(gctx),
            (name, "union-opt"))
        for f in FILTERS:
            _eq(eng.run_query(filter_plan(f)), filter_want(gctx, f), (name, f))


def _run_step(eng, case, remote=False):
    eng.begin_query(case.plan)
    eng.load_rbuf(case.table, case.v2c, 0)
    n = eng.execute_one_pattern_remote() if remote else \
        eng.execute_one_pattern()
    got = eng.fetch_raw()
    assert n == got.shape[0], (case.id, n, got.shape)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("d,mode", VU_MODES)
@pytest.mark.parametrize("config", list(STORE_ENVS))
def test_vu_step(gctx, engines, config, d, mode):
    """k_vu one step at a time: vertices with 1/63/64/65/130 predicates
    (the 64-lane inner stride), 4096 + 257 rows (the grid stride), vids
    below vp_base, past max_id and absent, both directions, both end
    modes, 1..7 input columns."""
    eng = engines[config]
    for case in vu_cases(gctx, d, mode):
        before = _launches(eng)
        got = _run_step(eng, case)
        _eq(got, case.ref(), case.id)
        assert _delta(eng, before)["expand"] == 1, case.id


@pytest.mark.gpu
def test_vu_plans(gctx, engines):
    for cname, eng in engines.items():
        for name, plan in vu_plans(gctx.meta).items():
            _eq(eng.run_query(plan), vu_plan_want(gctx, name), (cname, name))


@pytest.mark.gpu
def test_vu_disabled_store_raises(gctx):
    """A store built with WK_VERSATILE=0 has no predicate lists: the
    plan must be refused, not mis-executed."""
    with env(WK_VERSATILE=0):
        eng = wk.Engine(wk.Store(gctx.triples), device=0)
    for plan in vu_plans(gctx.meta).values():
        with pytest.raises(RuntimeError):
            eng.run_query(plan)
    # the engine still answers a plan without a predicate variable
    t = T_START[257]
    _eq(eng.run_query(opt_plan(gctx.meta, "k2u", t)),
        gctx.opt_want("k2u", t), "after-refusal")


def _split(eng, table, col, ndst, dev, cap_rows):
    n, ncols = table.shape
    eng.begin_query(split_plan(ncols, col))
    eng.load_rbuf(table, list(range(ncols)) + [-1], 0)
    counts = eng.generate_sub_query(ndst, dev, cap_rows)
    flat = wk.dev_download_u32(dev, n * ncols) if n else \
        np.empty(0, dtype=np.uint32)
    return counts, flat.reshape(n, ncols)


def _check_split(eng, table, col, ndst, dev, cap_rows, what):
    counts, out = _split(eng, table, col, ndst, dev, cap_rows)
    res = table[:, col] % ndst
    want = np.bincount(res, minlength=ndst)
    assert np.array_equal(np.array(counts), want), what
    lo = 0
    for d in range(ndst):
        chunk = out[lo:lo + want[d]]
        lo += want[d]
        assert (chunk[:, col] % ndst == d).all(), (what, d)
        assert np.array_equal(sort_rows(chunk), sort_rows(table[res == d])), \
            (what, d)
    # the engine's own table is untouched
    assert np.array_equal(eng.fetch_raw().reshape(table.shape), table), what


@pytest.mark.gpu
@pytest.mark.parametrize("ndst", NDST)
def test_split(engines, ndst):
    """generate_sub_query: counts, per-destination chunks as multisets
    and the untouched input, for 1..64 destinations, rows around the
    256-row block, 1/2/4/7 columns with every split column, uniform and
    fully skewed values."""
    eng = engines["default"]
    cap = max(ROWS)
    dev = wk.dev_alloc(cap * 7 * 4)
    try:
        before = _launches(eng)
        for n, c, col, pat in split_cases(ndst):
            _check_split(eng, split_table(n, c, col, ndst, pat), col, ndst,
                         dev, cap, (ndst, n, c, col, pat))
        assert _delta(eng, before)["split"] > 0
    finally:
        wk.dev_free(dev)


@pytest.mark.gpu
def test_split_many_chunks_and_refusals(engines):
    """1024 * 256 + 257 rows: each of the 1024 blocks walks its chunk in
    more than one 256-row trip.  ndst outside 1..64 and a destination
    buffer smaller than the table are refused."""
    eng = engines["default"]
    dev = wk.dev_alloc(SPLIT_BIG * 2 * 4)
    try:
        for ndst, pat in ((7, "uniform"), (64, "ends")):
            _check_split(eng, split_table(SPLIT_BIG, 2, 1, ndst, pat), 1,
                         ndst, dev, SPLIT_BIG, (ndst, pat))
        t = split_table(257, 2, 1, 2, "uniform")
        for ndst in (0, 65):
            eng.begin_query(split_plan(2, 1))
            eng.load_rbuf(t, [0, 1, -1], 0)
            with pytest.raises((RuntimeError, ValueError)):
                eng.generate_sub_query(ndst, dev, SPLIT_BIG)
        eng.begin_query(split_plan(2, 1))
        eng.load_rbuf(t, [0, 1, -1], 0)
        with pytest.raises(RuntimeError):
            eng.generate_sub_query(2, dev, 256)
        # and the engine still splits
        _check_split(eng, t, 1, 2, dev, SPLIT_BIG, "after-refusal")
    finally:
        wk.dev_free(dev)


@pytest.fixture(scope="module")
def peer_engines(ectx):
    """Engines over a store that imported itself as its only peer: the
    local branch of import_peers, no IPC handle opened."""
    out = {}
    for name, kv in STORE_ENVS.items():
        with env(**kv):
            store = wk.Store(ectx.triples)
            gstore = wk.GpuStore(store, device=0)
        try:
            blob = gstore.export_blob()
        except RuntimeError as e:
            pytest.skip("export_blob unavailable on this machine: %s" % e)
        gstore.import_peers([blob], [store.seg_table()])
        with env(**TIMED):
            out[name] = wk.Engine(gstore)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("op", list(T.OPS))
@pytest.mark.parametrize("config", list(STORE_ENVS))
def test_peer_step(ectx, peer_engines, config, op):
    """k_peer_step with one server against step_ref: the carry across
    256-row tiles, PM_SIZE / PM_COL / PM_CONST, the dense type lookup
    and its 0xFFFF fall-through to the probe."""
    eng = peer_engines[config]
    for case in peer_cases(ectx, op):
        before = _launches(eng)
        got = _run_step(eng, case, remote=True)
        _eq(got, case.ref(), case.id)
        d = _delta(eng, before)
        assert d["probe"] == 1 and d["expand"] == d["filter"] == 0, case.id


@pytest.mark.gpu
def test_peer_step_empty_segment_and_refusals(ectx, peer_engines):
    eng = peer_engines["default"]
    case = peer_cases(ectx, "k2u-deg")[4]
    assert case.n == 257
    s = -(case.col + 1)
    new = -(case.ncols + 1)

    def run(pat, remote=True):
        eng.begin_query(Plan([pat], nvars=case.ncols + 1, required_vars=[X]))
        eng.load_rbuf(case.table, case.v2c, 0)
        return eng.execute_one_pattern_remote()

    # predicates without a segment: inside and past the segment table
    for pid in (9, 1000):
        assert run((s, pid, OUT, new)) == 0
        assert run((s, pid, OUT, int(ectx.meta["pool"][0]))) == 0
    # shapes that must take the exchange path
    for pat in ((int(ectx.meta["ladder"][0]), sg.P_DEG, OUT, s),   # const start
                (s, TYPE, IN, new),                                # type index
                (s, new, OUT, int(ectx.meta["pool"][0]))):         # pred. var
        with pytest.raises(ValueError):
            run(pat)
    # still exact afterwards
    _eq(_run_step(eng, case, remote=True), case.ref(), case.id)


@pytest.fixture(scope="module")
def light_engine(lctx):
    with env(**TIMED):
        return wk.Engine(wk.Store(lctx.triples), device=0)


@pytest.mark.gpu
def test_light2_submit(lctx, light_engine):
    """submit + fetch_result of `c P ?x . ?x rdf:type T` on a store
    without multi-typed entities runs k_light2: lists of 0..1000 entries
    around the 64-lane and 256-thread strides, an id below type_base and
    the last vid."""
    eng, adj = light_engine, lctx.adj
    for c in list(lctx.meta["consts"]) + [lctx.meta["absent"]]:
        for cval in (LT_F, LT_O):
            want = sort_rows(light_ref(adj, c, P_L, OUT, cval)[:, None])
            plan = light_plan(c, cval)
            eng.submit(plan)
            _eq(eng.fetch_result(), want, (int(c), cval, "submit"))
            _eq(eng.run_query(plan), want, (int(c), cval, "run_query"))
    # the route: k_light2 adds `6 * list + 4 * kept` filter bytes after
    # it publishes the counters, so a second submit reports the first's
    c = lctx.meta["consts"][-1]
    n = len(adj[(int(c), P_L, OUT)])
    kept = len(light_ref(adj, c, P_L, OUT, LT_F))
    eng.submit(light_plan(c))
    eng.fetch_result()
    b0 = eng.kernel_stats()["filter"]["bytes"]
    eng.submit(light_plan(c))
    eng.fetch_result()
    b1 = eng.kernel_stats()["filter"]["bytes"]
    eng.submit(light_plan(c))
    eng.fetch_result()
    b2 = eng.kernel_stats()["filter"]["bytes"]
    assert b1 - b0 == b2 - b1 == 6 * n + 4 * kept, (b0, b1, b2, n, kept)


@pytest.mark.gpu
def test_light_batch(lctx, light_engine):
    """One k_light_batch window holding every constant, a nonexistent
    one and one constant under two filter types; two windows back to
    back; an ordinary query afterwards."""
    eng, adj, meta = light_engine, lctx.adj, lctx.meta
    consts = [int(c) for c in meta["consts"]]
    # the constant that goes in twice keeps different counts per type
    two = next(c for c in reversed(consts)
               if len(light_ref(adj, c, P_L, OUT, LT_F))
               != len(light_ref(adj, c, P_L, OUT, LT_O)))
    subj = consts + [meta["absent"], two, two]
    cval = [LT_F] * (len(consts) + 1) + [LT_F, LT_O]
    n = len(subj)
    want = [len(light_ref(adj, s, P_L, OUT, t)) for s, t in zip(subj, cval)]
    assert want[-1] != want[-2] and want[len(consts)] == 0
    before = _launches(eng)
    for _ in range(2):
        eng.submit_light_batch(subj, [P_L] * n, [OUT] * n, cval)   # no raise
        got = eng.wait_light_batch()
        assert got.tolist() == want
    # reversed order and the other type: per-query regions do not mix
    eng.submit_light_batch(subj[::-1], [P_L] * n, [OUT] * n, [LT_O] * n)
    got = eng.wait_light_batch()
    assert got.tolist() == [len(light_ref(adj, s, P_L, OUT, LT_O))
                            for s in subj[::-1]]
    assert _delta(eng, before)["filter"] == 3
    plan = light_plan(consts[-1])
    _eq(eng.run_query(plan),
        sort_rows(light_ref(adj, consts[-1], P_L, OUT, LT_F)[:, None]),
        "after-batch")


@pytest.mark.gpu
def test_light_refused_on_multi_typed_store(gctx, engines):
    """The counterpart: a multi-typed store refuses the batch."""
    with pytest.raises(ValueError):
        engines["default"].submit_light_batch([int(gctx.meta["c_list"])],
                                              [P_LIST], [OUT], [GT_B])


@pytest.mark.gpu
@pytest.mark.parametrize("ncols", [1, 4, 7])
def test_projection(engines, ncols):
    """fetch_result of one loaded 257-row table: k_project for up to 8
    required vars (permuted, repeated, one without a column), the host
    projection for 9 and for more required vars than the table buffers
    have columns."""
    eng = engines["default"]
    table = proj_table(ncols)
    nv = ncols + 1
    pats = [(X, P_OPT, OUT, -nv)]
    eng.begin_query(Plan(pats, nv, [X]))
    eng.load_rbuf(table, list(range(ncols)) + [-1], 1)
    for name, req in proj_cases(ncols).items():
        before = _launches(eng)
        got = eng.fetch_result(Plan(pats, nv, req))
        want = proj_want(table, req)
        assert got.shape == want.shape, (name, got.shape)
        assert np.array_equal(got, want), name         # row order is kept
        if len(req) <= nv:
            assert _delta(eng, before)["other"] == 1, name
    assert np.array_equal(eng.fetch_raw(), table)


# a fresh engine per case: capacities only grow
_CAP_CHILD = """
import os, sys
os.environ['WK_MIN_CAP'] = '1000'
sys.path.insert(0, %r)
mode = %r
import numpy as np
import wukong_amd as wk
from tests import group_graph as gg
from tests import test_gpu_group_edges as G
from tests.oracle_util import sort_rows
if mode == 'peer':
    cx = G.T.Ctx()
    store = wk.Store(cx.triples)
    gstore = wk.GpuStore(store, device=0)
    gstore.import_peers([gstore.export_blob()], [store.seg_table()])
    ran = 0
    for case in G.peer_cases(cx, 'k2u-hub'):
        if case.n < 255:
            continue
        assert len(case.ref()) > 1000, case.id
        G._eq(G._run_step(wk.Engine(gstore), case, remote=True), case.ref(),
              case.id)
        ran += 1
    assert ran >= 6
else:
    cx = G.GCtx(*gg.group_graph())
    gstore = wk.GpuStore(wk.Store(cx.triples), device=0)
    if mode == 'optional':
        for group in ('k2u', 'k2u-type', 'k2u-k2u-type', 'k2k'):
            for n in (255, 257, 1025):
                t = gg.T_START[n]
                want = cx.opt_want(group, t)
                assert len(want) > 1000
                G._eq(wk.Engine(gstore).run_query(
                    G.opt_plan(cx.meta, group, t)), want, (group, n))
    else:
        for d, m in G.VU_MODES:
            for case in G.vu_cases(cx, d, m):
                if case.n not in (255, 257, 1025):
                    continue
                assert len(case.ref()) > 1000, case.id
                G._eq(G._run_step(wk.Engine(gstore), case), case.ref(),
                      case.id)
        want = G.vu_plan_want(cx, 'k2uu-out')
        assert len(want) > 1000
        G._eq(wk.Engine(gstore).run_query(G.vu_plans(cx.meta)['k2uu-out']),
              want, 'k2uu-out')
print('GROUP_CAP_OK', mode)
"""


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["optional", "vu", "peer"])
def test_capacity_rerun(mode):
    """WK_MIN_CAP=1000 in a child process: the 300-edge rows overflow
    inside the OPTIONAL group (the whole query re-runs), k_vu overruns
    S_TOTAL (the step re-runs) and the P_HUB ladder overflows on the
    remote path (the re-run stays remote); all still exact."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CAP_CHILD % (root, mode)],
                       capture_output=True, text=True, timeout=300)
    assert "GROUP_CAP_OK " + mode in r.stdout, r.stdout + r.stderr
