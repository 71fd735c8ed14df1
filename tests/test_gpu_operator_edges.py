"""Operator-level edge tests on the synthetic graph of synth_graph.py.

The LUBM/WatDiv parity tests only reach the degrees, row counts, hash
occupancy and type layout those generators produce.  Here every
operator runs one step at a time, and as whole plans, over a graph that
has a row on each hard threshold of the kernels (see synth_graph.py),
with exact comparisons against references that share no code with the
engine.

CPU part (unmarked): the graph's invariants, oracle == brute for every
whole plan, step_ref == OracleExecutor for every step case — the
references are validated against each other here.  GPU part: the engine
against those references only.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import wukong_amd as wk
from wukong_amd import Plan
from tests import oracle_util
from tests import synth_graph as sg
from tests.oracle_util import OracleCtx, OracleExecutor, sort_rows
from tests.synth_graph import (B, IN, OUT, TYPE, P_DEG, P_HUB, P_FN, P_RFN,
                               P_CHAIN, P_LP, T_A, T_B, T_C, T_N1, T_N2, T_OD,
                               T_F1, T_F2, T_F3, LP_CAP, env, step_ref)

ROWS = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049]
NCOLS = [1, 2, 4, 7]
# smallest input at which one block's chunk of the 2048-block scan grid
# exceeds the 256-row tile (multi-tile carry), with a partial last tile
BIG = 2048 * 256 + 257

# store configurations of the GPU part: WK_* set while the store builds
STORE_ENVS = {
    "default": {},
    "hash": dict(WK_FN=0, WK_CSR=0, WK_TBM=0),   # cluster hash + type_of
    "notbm": dict(WK_TBM=0),
}
# engine configurations: (store, WK_* set around every call)
CONFIGS = {
    "default": ("default", {}),
    "default-nofn": ("default", dict(WK_FN_DISPATCH=0)),
    "hash": ("hash", {}),
    "notbm": ("notbm", {}),
}


class Ctx:
    """The graph, its plain adjacency and the shared oracle."""

    def __init__(self):
        self.triples, self.meta = sg.edge_graph()
        self.adj = sg.adjacency(self.triples)
        self.ora = OracleCtx(self.triples)
        self._want = {}

    def want(self, name, plan):
        """Oracle rows of a whole plan, sorted, computed once."""
        if name not in self._want:
            self._want[name] = sort_rows(self.ora.run_query(plan))
        return self._want[name]


@pytest.fixture(scope="module")
def ctx():
    return Ctx()


# ---------------------------------------------------------------------
# whole plans
# ---------------------------------------------------------------------
def _typed_plan(t_start, pid):
    return Plan([(t_start, TYPE, IN, -1), (-1, pid, OUT, -2),
                 (-2, TYPE, OUT, T_B)], nvars=2, required_vars=[-1, -2])


# <start type> type-IN ?x . ?x P ?y . ?y type T_B
PLANS = {
    # ladder subjects: rows with 32/33, 64/65 ... 5000 edges, objects of
    # every type class (the filter drops about 2/7)
    "deg-ladder": _typed_plan(T_A, P_DEG),
    "hub-ladder": _typed_plan(T_A, P_HUB),
    # every object is single-typed T_B: the filter drops nothing
    "deg-nodrop": _typed_plan(T_N1, P_DEG),
    "hub-nodrop": _typed_plan(T_N1, P_HUB),
    # exactly one object (in a 34-edge row) is not T_B
    "deg-onedrop": _typed_plan(T_OD, P_DEG),
    "hub-onedrop": _typed_plan(T_OD, P_HUB),
    "fn-nodrop": _typed_plan(T_F1, P_FN),
    "fn-drop": _typed_plan(T_F2, P_FN),
}
# no-drop plans whose new column holds a multi-typed entity that HAS the
# filter type: without type bitmaps the optimistic replay must miss
MISS_PLANS = {
    "fn-multi": _typed_plan(T_F3, P_FN),
    "hub-multi": _typed_plan(T_N2, P_HUB),
    "deg-multi": _typed_plan(T_N2, P_DEG),
}


def _lp_plans(meta):
    """LDS-interpreter templates: name -> (template, consts)."""
    c, m, d = meta["lp_c"], meta["lp_m"], meta["lp_d"]
    absent = meta["absent"]
    one = Plan([(int(c[0]), P_LP, OUT, -1)], nvars=1, required_vars=[-1])
    two = Plan([(int(d[0]), P_LP, OUT, -1), (-1, P_LP, OUT, -2)], nvars=2,
               required_vars=[-1, -2])
    typed = Plan([(int(m[0]), P_LP, OUT, -1), (-1, TYPE, OUT, T_B)], nvars=1,
                 required_vars=[-1])
    return {
        "one": (one, [int(x) for x in c] + [absent, int(m[1])]),
        "two": (two, [int(d[0]), int(d[1]), int(m[0]), int(c[1]), absent]),
        "typed": (typed, [int(m[0]), int(m[2]), int(c[1]), int(c[2]), absent]),
    }


def _with_const(tmpl, const):
    pats = list(tmpl.patterns)
    pats[0] = (int(const),) + tuple(pats[0][1:])
    return Plan(pats, tmpl.nvars, tmpl.required_vars)


# ---------------------------------------------------------------------
# single-operator step cases
# ---------------------------------------------------------------------
# name -> (mode, pid, dir, which meta values lead the start column,
#          const picker for k2c)
OPS = {
    "k2u-deg": ("k2u", P_DEG, OUT, "ladder", None),
    "k2u-hub": ("k2u", P_HUB, OUT, "ladder", None),
    "k2u-fn": ("k2u", P_FN, OUT, "fn", None),
    "k2u-chain": ("k2u", P_CHAIN, OUT, "chain", None),
    "k2k-deg": ("k2k", P_DEG, OUT, "ladder", None),
    "k2k-chain": ("k2k", P_CHAIN, OUT, "chain", None),
    "k2k-fn": ("k2k", P_FN, OUT, "fn", None),
    "k2k-rfn": ("k2k", P_RFN, OUT, "rfn_s", None),       # fn_swap
    # pool[31] is the LAST edge of the 32-edge row, absent from the
    # 31-edge row
    "k2c-deg": ("k2c", P_DEG, OUT, "ladder", lambda m: m["pool"][31]),
    "k2c-chain": ("k2c", P_CHAIN, OUT, "chain", lambda m: m["nb"][21]),
    "k2c-fn": ("k2c", P_FN, OUT, "fn", lambda m: m["nb"][2]),
    "k2c-rfn": ("k2c", P_RFN, OUT, "rfn_s", lambda m: m["rfn_o"][1]),  # PM_EQ
    # const with no IN edge: the host-resolved vertex is 0, nothing kept
    "k2c-rfn-none": ("k2c", P_RFN, OUT, "rfn_s", lambda m: m["pool"][0]),
    "type-b": ("k2c", TYPE, OUT, "typed", lambda m: T_B),
    "type-a": ("k2c", TYPE, OUT, "typed", lambda m: T_A),
}
BIG_OPS = ["k2u-deg", "k2u-fn", "k2c-fn", "type-b"]


def _start_values(meta, lead, big):
    """Start-column values: the operator's own keys first, then every
    other special vertex.  Big tables keep to degree <= 2 keys."""
    edge = [meta["absent"]] + meta["sub_base"] + [meta["max_id"],
                                                 meta["past_max"]]
    typed = list(meta["pool"][:8]) + [meta["multi"], meta["bad"]] + \
        list(meta["nb"][:2]) + list(meta["lpo"][:5])
    if big:
        # pool vertices have no OUT edge of these predicates; they give
        # the type filter a keep rate that exercises its compaction
        vals = list(meta["fn"]) + list(meta["fn_gaps"]) + edge + \
            list(meta["filler"]) + typed + list(meta["pool"][:3000])
        return np.array(vals, dtype=np.uint32)
    parts = dict(
        ladder=list(meta["ladder"]), fn=list(meta["fn"]) + list(meta["fn_gaps"]),
        chain=list(meta["chain"]), rfn_s=list(meta["rfn_s"]), typed=typed)
    vals = parts.pop(lead) + edge
    for k in ("ladder", "fn", "chain", "rfn_s", "typed"):
        vals += parts.get(k, [])
    for subj in meta["groups"].values():
        vals += list(subj)
    vals += list(meta["rfn_o"]) + list(meta["filler"][:4])
    return np.array(vals, dtype=np.uint32)


class StepCase:
    def __init__(self, cx, op, n, ncols, col, big=False, choose=None):
        """`choose` maps the start values to the ones to use (the partition
        tests keep the values one rank owns)."""
        mode, pid, d, lead, pick = OPS[op]
        self.op, self.n, self.ncols, self.col = op, n, ncols, col
        self.mode, self.pid, self.d = mode, pid, d
        self.id = "%s-n%d-c%d" % (op, n, ncols)
        meta = cx.meta
        vals = _start_values(meta, lead, big)
        if choose is not None:
            vals = choose(vals)
        r = np.arange(n, dtype=np.int64)
        t = np.empty((n, ncols), dtype=np.uint32)
        for j in range(ncols):
            t[:, j] = B + (r * (j + 3) + j) % 1000
        t[:, col] = np.resize(vals, n) if n else vals[:0]
        self.col2, self.const = None, None
        if mode == "k2k":
            self.col2 = (col + 1) % ncols
            # two rows in three aim at a real neighbour, the rest miss
            L = 3 * len(vals)
            blk = np.empty(L, dtype=np.uint32)
            for i in range(L):
                lst = cx.adj.get((int(vals[i % len(vals)]), pid, d))
                if lst is not None and i % 3 != 2:
                    blk[i] = lst[(i * 7) % len(lst)]
                else:
                    blk[i] = meta["pool"][i % 50]
            t[:, self.col2] = np.resize(blk, n) if n else blk[:0]
        elif mode == "k2c":
            self.const = int(pick(meta))
        self.table = t
        s = -(col + 1)
        if mode == "k2u":
            self.plan = Plan([(s, pid, d, -(ncols + 1))], nvars=ncols + 1,
                             required_vars=[-1])
            self.v2c = list(range(ncols)) + [-1]
        else:
            o = -(self.col2 + 1) if mode == "k2k" else self.const
            self.plan = Plan([(s, pid, d, o)], nvars=ncols,
                             required_vars=[-1])
            self.v2c = list(range(ncols))
        self._ref = None
        self._cx = cx

    def ref(self):
        """step_ref rows, sorted, computed once and left unchanged."""
        if self._ref is None:
            self._ref = sort_rows(step_ref(
                self.table, self.col, self._cx.adj, self.mode, self.pid,
                self.d, col2=self.col2, const=self.const))
            self._ref.setflags(write=False)
        return self._ref


_CASES = {}


def step_cases(cx, op):
    if op not in _CASES:
        widths = [c for c in NCOLS if c >= (2 if OPS[op][0] == "k2k" else 1)]
        cases = []
        for i, n in enumerate(ROWS):
            c = widths[i % len(widths)]
            cases.append(StepCase(cx, op, n, c, i % c))
        have = {(k.n, k.ncols) for k in cases}
        for c in widths:       # every column count at one odd row count
            if (257, c) not in have:
                cases.append(StepCase(cx, op, 257, c, c - 1))
        if op in BIG_OPS:
            cases.append(StepCase(cx, op, BIG, 2, 1, big=True))
        _CASES[op] = cases
    return _CASES[op]


# ---------------------------------------------------------------------
# CPU part
# ---------------------------------------------------------------------
def test_graph_store_invariants(ctx):
    meta = ctx.meta
    assert 60000 <= len(ctx.triples) <= 80000
    assert ctx.triples.dtype == np.uint32
    assert int(ctx.triples[:, [0, 2]].max()) == meta["max_id"]
    store = wk.Store(ctx.triples)
    assert store.check() == 0
    # either side of the type-fused CSR gate (edges / keys <= 32)
    k, e = store.seg_stats(P_DEG, OUT)
    assert k > 0 and e / k <= 32 and e // k <= 32
    k, e = store.seg_stats(P_HUB, OUT)
    assert k > 0 and e // k > 32
    # functional exactly where designed
    k, e = store.seg_stats(P_FN, OUT)
    assert k == e == len(meta["fn"])
    k, e = store.seg_stats(P_FN, IN)
    assert 0 < k < e
    k, e = store.seg_stats(P_RFN, IN)
    assert k == e == len(meta["rfn_o"])
    k, e = store.seg_stats(P_RFN, OUT)
    assert 0 < k < e
    # ladder degrees as designed, on both predicates
    for s, d in zip(meta["ladder"], meta["ladder_degs"]):
        assert len(store.get_triples(int(s), P_DEG, OUT)) == d
        assert len(store.get_triples(int(s), P_HUB, OUT)) == d
    # LDS-interpreter list sizes
    assert [len(store.get_triples(int(c), P_LP, OUT)) for c in meta["lp_c"]] \
        == [LP_CAP - 1, LP_CAP, LP_CAP + 1]
    for d, total in zip(meta["lp_d"], (LP_CAP // 2, LP_CAP // 2 + 1)):
        mids = store.get_triples(int(d), P_LP, OUT)
        assert sum(len(store.get_triples(int(m), P_LP, OUT))
                   for m in mids) == total
    # multi-typed, untyped and single-typed entities all exist
    assert list(store.get_triples(meta["multi"], TYPE, OUT)) == [T_A, T_B]
    assert len(store.get_triples(int(meta["pool"][2]), TYPE, OUT)) == 0
    assert list(store.get_triples(int(meta["nb"][0]), TYPE, OUT)) == [T_B]


def test_chain_collisions(ctx):
    """40 P_CHAIN keys -> 8 buckets of 7 slots + chain: 22 keys in one
    bucket walk three chained buckets, 16 in another walk two.  The
    bucket of each key is recomputed with the oracle's own hash."""
    meta = ctx.meta
    chain = meta["chain"]
    assert len(chain) == sg.N_CHAIN and len(set(chain.tolist())) == sg.N_CHAIN
    store = wk.Store(ctx.triples)
    k, _ = store.seg_stats(P_CHAIN, OUT)
    assert k == sg.N_CHAIN and (k + 4) // 5 == sg.CHAIN_BUCKETS
    occ = np.zeros(sg.CHAIN_BUCKETS, dtype=int)
    for v in chain:
        key = oracle_util.key_pack(int(v), P_CHAIN, OUT)
        assert key == wk.key_pack(int(v), P_CHAIN, OUT)
        h = oracle_util.hash_u64(key)
        assert h == wk.hash_u64(key)
        occ[h % sg.CHAIN_BUCKETS] += 1
    assert occ[meta["chain_long_bucket"]] == sg.CHAIN_LONG == 22
    assert occ[meta["chain_mid_bucket"]] == sg.CHAIN_MID == 16
    assert sg.CHAIN_LONG > 3 * 7 and 2 * 7 < sg.CHAIN_MID <= 3 * 7
    for v in chain:
        want = ctx.adj[(int(v), P_CHAIN, OUT)]
        assert np.array_equal(store.get_triples(int(v), P_CHAIN, OUT), want)
        assert np.array_equal(ctx.ora.get_triples(int(v), P_CHAIN, OUT), want)


@pytest.mark.parametrize("name", list(PLANS) + list(MISS_PLANS))
def test_plans_oracle_vs_brute(ctx, name):
    plan = {**PLANS, **MISS_PLANS}[name]
    want = ctx.want(name, plan)
    assert want.shape[0] > 0
    assert np.array_equal(want, sort_rows(ctx.ora.brute_query(plan)))


def test_plan_shapes(ctx):
    """The drop behaviour each plan was built for, on the plain
    adjacency: no-drop plans keep every expanded row, one-drop plans
    lose exactly one, the multi-typed plans keep a multi-typed entity."""
    adj, meta = ctx.adj, ctx.meta
    members = {}
    for s, p, o in ctx.triples.tolist():
        if p == TYPE:
            members.setdefault(o, set()).add(s)

    def counts(plan):
        t_start, pid = plan.patterns[0][0], plan.patterns[1][1]
        objs = [int(o) for s in sorted(members[t_start])
                for o in adj.get((s, pid, OUT), [])]
        return len(objs), sum(o in members[T_B] for o in objs), objs

    for name in ("deg-nodrop", "hub-nodrop", "fn-nodrop"):
        n, kept, _ = counts(PLANS[name])
        assert n == kept > 0, name
    for name in ("deg-onedrop", "hub-onedrop"):
        n, kept, _ = counts(PLANS[name])
        assert n == kept + 1, name
    for name in ("deg-ladder", "hub-ladder", "fn-drop"):
        n, kept, _ = counts(PLANS[name])
        assert 0 < kept < n, name
    for name, plan in MISS_PLANS.items():
        n, kept, objs = counts(plan)
        assert n == kept > 0 and meta["multi"] in objs, name
    for name, plan in {**PLANS, **MISS_PLANS}.items():
        assert len(ctx.want(name, plan)) == counts(plan)[1], name


def test_lp_plans_oracle_vs_brute(ctx):
    for name, (tmpl, consts) in _lp_plans(ctx.meta).items():
        for c in consts:
            plan = _with_const(tmpl, c)
            a = sort_rows(ctx.ora.run_query(plan))
            b = sort_rows(ctx.ora.brute_query(plan))
            assert a.shape == b.shape and np.array_equal(a, b), (name, c)


@pytest.mark.parametrize("op", list(OPS))
def test_step_ref_vs_oracle(ctx, op):
    for case in step_cases(ctx, op):
        ex = OracleExecutor(ctx.ora, case.plan)
        ex.load(case.table, case.v2c, 0)
        ex.step()
        got = sort_rows(ex.table())
        want = case.ref()
        assert got.shape == want.shape, (case.id, got.shape, want.shape)
        assert np.array_equal(got, want), case.id
        if case.n >= 255 and case.op not in ("k2c-rfn-none",):
            assert 0 < len(want), case.id   # the case is not vacuous
        if case.mode != "k2u" and case.n >= 255:
            assert len(want) < case.n, case.id


# ---------------------------------------------------------------------
# GPU part
# ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def engines(ctx):
    """One store + engine per store configuration, built once."""
    out = {}
    for name, kv in STORE_ENVS.items():
        with env(**kv):
            out[name] = wk.Engine(wk.Store(ctx.triples), device=0)
    return out


def _engine(engines, config):
    store, kv = CONFIGS[config]
    return engines[store], kv


def _run_step(eng, case):
    eng.begin_query(case.plan)
    eng.load_rbuf(case.table, case.v2c, 0)
    n = eng.execute_one_pattern()
    got = eng.fetch_raw()
    assert n == got.shape[0], (case.id, n, got.shape)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("op", list(OPS))
@pytest.mark.parametrize("config", list(CONFIGS))
def test_step_operator(ctx, engines, config, op):
    """begin_query -> load_rbuf -> execute_one_pattern -> fetch_raw of
    one operator against step_ref: row counts around the 256-row scan
    tile, the 1024-row filter tile and the 2048-block grid, 1/2/4/7
    input columns, and (BIG_OPS) the multi-tile scan carry."""
    eng, kv = _engine(engines, config)
    with env(**kv):
        for case in step_cases(ctx, op):
            got = _run_step(eng, case)
            want = case.ref()
            assert got.shape == want.shape, (case.id, got.shape, want.shape)
            assert np.array_equal(sort_rows(got), want), case.id


def _check_plan(eng, ctx, name, plan):
    want = ctx.want(name, plan)
    got = eng.run_query(plan)
    assert got.shape == want.shape, (name, "run_query", got.shape, want.shape)
    assert np.array_equal(sort_rows(got), want), (name, "run_query")
    eng.submit(plan)
    got = eng.fetch_result()
    assert got.shape == want.shape, (name, "submit", got.shape, want.shape)
    assert np.array_equal(sort_rows(got), want), (name, "submit")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PLANS))
@pytest.mark.parametrize("config", list(CONFIGS))
def test_whole_plans(ctx, engines, config, name):
    """run_query, submit + fetch_result and graph replay (twice) of each
    plan against the oracle.  On the default store the P_DEG plans take
    the type-fused CSR path (rows with > 32 and > 64 edges) and the
    P_HUB plans may not; in a capture the no-drop plans select the
    verify-fused expansion, the verify-only filter and k_expand_fn_map,
    the dropping ones the compacting kernels."""
    eng, kv = _engine(engines, config)
    plan = PLANS[name]
    with env(**kv):
        _check_plan(eng, ctx, name, plan)
        gid = eng.graph_build(plan)
        for _ in range(2):
            assert eng.graph_run(gid) == len(ctx.want(name, plan)), name
        # the engine is still good for the plain path after replays
        _check_plan(eng, ctx, name, plan)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MISS_PLANS))
def test_optimistic_miss_fallback(ctx, engines, name):
    """No-drop plans whose new column holds a multi-typed entity that
    has the filter type.  Without type bitmaps the optimistic kernels
    (k_expand_fn_map, verify-fused k_expand_in/k_expand_big) read
    type_of == 0xFFFF as a miss: the replay must be discarded
    (OverflowError) or be right — never a wrong count — and the safe
    path must then give the oracle rows.  With bitmaps the replay is
    exact."""
    plan = MISS_PLANS[name]
    want = ctx.want(name, plan)
    for store in ("notbm", "hash"):
        eng = engines[store]
        gid = eng.graph_build(plan)
        for _ in range(2):
            try:
                n = eng.graph_run(gid)
            except OverflowError:
                n = None
            assert n is None or n == len(want), (name, store, n, len(want))
            _check_plan(eng, ctx, name, plan)
    eng = engines["default"]
    gid = eng.graph_build(plan)
    for _ in range(2):
        assert eng.graph_run(gid) == len(want), name
    _check_plan(eng, ctx, name, plan)


_CAP_CHILD = """
import os, sys
os.environ['WK_MIN_CAP'] = '1000'
sys.path.insert(0, %r)
import numpy as np
import wukong_amd as wk
from tests import synth_graph as sg
from tests import test_gpu_operator_edges as T
from tests.oracle_util import OracleCtx, sort_rows
triples, meta = sg.edge_graph()
ora = OracleCtx(triples)
with sg.env(**T.STORE_ENVS['hash']):
    gstore = wk.GpuStore(wk.Store(triples), device=0)
plans = dict(T.PLANS)
plans.update(T.MISS_PLANS)
for name, plan in plans.items():
    if not name.startswith('hub-'):
        continue
    want = sort_rows(ora.run_query(plan))
    # capacities only grow: a fresh engine per path starts at 1000 rows
    got = wk.Engine(gstore).run_query(plan)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert np.array_equal(sort_rows(got), want), name
    # step API: the mid-plan overflow re-run from the intact input table
    eng = wk.Engine(gstore)
    eng.begin_query(plan)
    for _ in plan.patterns:
        eng.execute_one_pattern()
    got = eng.fetch_result()
    assert got.shape == want.shape, (name, 'step', got.shape, want.shape)
    assert np.array_equal(sort_rows(got), want), (name, 'step')
print('CAP_TRUNCATION_OK')
"""


@pytest.mark.gpu
def test_capacity_truncation():
    """WK_MIN_CAP=1000 on the hash-only store: the 5000-edge row of the
    P_HUB plans straddles the capacity, so k_expand_in / k_expand_big
    clamp at `basep + deg > cap`, the step flags S_ERR, the engine grows
    and re-runs — results must still be exact."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CAP_CHILD % (root,)],
                       capture_output=True, text=True, timeout=300)
    assert "CAP_TRUNCATION_OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("store", ["default", "hash"])
def test_capacity_ends_inside_a_queued_row(ctx, engines, store):
    """WK_MIN_CAP=16 on the three- and four-row start sets of the P_DEG
    plans: the first row fits, the capacity ends inside the next one (33
    edges of T_N1, 34 of T_OD: the one-wave-per-row pass clamps at
    `pos < cap`) and the rows behind it start past the capacity.  On the
    default store that is the type-fused writer pair (k_expand_tf /
    k_expand_tf_big), on the hash store k_probe_scan + k_expand_in /
    k_expand_big.  The first fetch reports the overflow; the re-run at
    the grown capacity is exact."""
    with env(WK_MIN_CAP=16, **STORE_ENVS[store]):
        for name in ("deg-nodrop", "deg-onedrop"):
            plan, want = PLANS[name], ctx.want(name, PLANS[name])
            assert len(want) > 16 + 33
            eng = wk.Engine(engines[store]._store, device=0)
            eng.submit(plan)
            assert eng.fetch_count() < 0, name
            got = eng.run_query(plan)
            assert got.shape == want.shape, (name, got.shape, want.shape)
            assert np.array_equal(sort_rows(got), want), name


@pytest.mark.gpu
def test_plan_batch_capacity_boundary(ctx, engines):
    """LDS plan interpreter at LP_CAP: a c2u list of LP_CAP - 1 and
    LP_CAP edges fits, LP_CAP + 1 overflows; a c2u -> k2u table of
    LP_CAP / 2 two-column rows fits, one more row overflows.  Every
    other entry equals the oracle count.  The rdf:type template runs on
    a multi-typed graph, so it takes the K2C hash path."""
    eng = engines["default"]
    meta = ctx.meta
    ovf = np.uint64(wk.LP_OVERFLOW)
    counts = {}
    for name, (tmpl, consts) in _lp_plans(meta).items():
        eng.submit_plan_batch(tmpl, consts)
        got = eng.wait_light_batch()
        counts[name] = got
        for c, n in zip(consts, got):
            if n != ovf:
                want = len(ctx.ora.run_query(_with_const(tmpl, c)))
                assert n == want, (name, c, int(n), want)
    assert list(counts["one"][:3]) == [LP_CAP - 1, LP_CAP, ovf]
    assert list(counts["one"][3:]) == [0, LP_CAP // 2 - 3000]
    # (rows) * 2 == LP_CAP passes, one more row overflows; a LP_CAP-row
    # first column whose k2u finds nothing is not an overflow
    assert list(counts["two"]) == [LP_CAP // 2, ovf, 0, 0, 0]
    assert counts["typed"][3] == ovf and not np.any(counts["typed"][:3] == ovf)
    assert counts["typed"][0] > 0 and counts["typed"][4] == 0
