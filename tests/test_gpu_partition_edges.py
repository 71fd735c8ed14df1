"""Operator edge tests on PARTITIONED stores (nsrv = 2, 3, 8).

The other edge modules build every store with nsrv=1.  The multi-GPU
driver runs the engine on `wk.Store(triples, sid=r, nsrv=W)`, where the
side indexes (type_of, type bitmaps, functional maps, CSR) are built per
partition and the host-side `nsrv == 1` guards switch fast paths off.
Here every rank of W = 2, 3 and 8 runs in ONE process (tests/part_loop.py):
single steps on the keys a rank owns, the unsplit table on every rank,
whole plans through an in-process loopback of the distributed driver,
the caller-supplied list filter, and the whole-plan entry points on one
partition.

CPU part (unmarked): the partitions hold what they should, the
partition-local conditions the GPU cases rely on exist (seg_stats), the
per-rank step references equal the partition oracle, and the loopback
over oracle executors equals the single-partition oracle.  GPU part: the
engines against those references only, exactly.

Partition conditions of edge_graph(), as asserted below:
  * (P_RFN, OUT) and (P_FN, IN) are functional on some rank of every W
    and on no full store: W=2 rank 1, W=3 rank 2 (and rank 0 for P_FN
    IN), W=8 rank 5 (P_RFN OUT) and ranks 0, 1, 3, 4 (P_FN IN);
  * P_DEG OUT stays at or below 32 edges per key on every rank and P_HUB
    OUT above it on every rank: both sides of the gate occur for every
    W, but no partition moves a predicate across it, so the gate never
    decides differently from the full store there.  gate_graph() adds the
    few triples that put one rank of W=8 on the other side;
  * an empty P_RFN segment exists for W=8 only (OUT on ranks 0-3 and 7,
    IN on ranks 5 and 6); W=2 and W=3 leave no P_CHAIN / P_RFN segment
    empty, so that condition is asserted for W=8.
"""
import gc

import numpy as np
import pytest

import wukong_amd as wk
from wukong_amd import Plan
from tests import filter_ref
from tests import group_graph as gg
from tests import part_loop as pl
from tests import synth_graph as sg
from tests import test_gpu_chain_fusion as CF
from tests import test_gpu_operator_edges as T
from tests.oracle_util import OracleCtx, OracleExecutor, sort_rows
from tests.synth_graph import (B, IN, OUT, TYPE, P_DEG, P_HUB, P_FN, P_RFN,
                               P_CHAIN, LP_CAP, env, step_ref)

WS = [2, 3, 8]
ROWS, NCOLS, BIG = T.ROWS, T.NCOLS, T.BIG
X, Y = -1, -2
STORE_ENVS = {"default": {}, "hash": dict(WK_FN=0, WK_CSR=0, WK_TBM=0)}
# (W, store configuration) of the GPU part
PARTS = [(3, "default"), (3, "hash"), (2, "default"), (8, "default")]
TIMED = dict(WK_KERNEL_TIMING=1)
BIG_W, BIG_RANK = 3, 2      # rank 2 owns the P_FN keys of k2c-fn
EMPTY_SEG_W = 8        # the only W that leaves a P_RFN segment empty
# W -> (rank, pid, dir) of the segments that are functional on the
# partition and not on the full store
LOCAL_FN = {
    2: [(1, P_FN, IN), (1, P_RFN, OUT)],
    3: [(0, P_FN, IN), (2, P_FN, IN), (2, P_RFN, OUT)],
    8: [(0, P_FN, IN), (1, P_FN, IN), (3, P_FN, IN), (4, P_FN, IN),
        (5, P_RFN, OUT)],
}
# W -> (rank, pid, dir) of the empty P_CHAIN / P_RFN segments
EMPTY_SEGS = {8: [(r, P_RFN, OUT) for r in (0, 1, 2, 3, 7)] +
              [(5, P_RFN, IN), (6, P_RFN, IN)]}


def _same(got, want):
    """Exact equality of two sorted row sets (an empty result has no
    column count worth comparing)."""
    if len(got) == 0 or len(want) == 0:
        return len(got) == len(want)
    return got.shape == want.shape and np.array_equal(got, want)


# ---------------------------------------------------------------------
# graphs, plans and their single-partition references
# ---------------------------------------------------------------------
class GroupCtx:
    def __init__(self):
        self.triples, self.meta = gg.group_graph()
        self.ora = OracleCtx(self.triples)


class GateCtx:
    def __init__(self):
        self.triples, self.meta = sg.gate_graph()
        self.adj = sg.adjacency(self.triples)
        self.ora = OracleCtx(self.triples)


class LightCtx:
    def __init__(self):
        self.triples, self.meta = gg.single_typed_graph()
        self.ora = OracleCtx(self.triples)


_GRAPHS = {}


def graph(name):
    """'edge' | 'group' | 'chain' | 'gate' | 'light': built once per
    session."""
    if name not in _GRAPHS:
        _GRAPHS[name] = {"edge": T.Ctx, "group": GroupCtx, "chain": CF.Ctx,
                         "gate": GateCtx, "light": LightCtx}[name]()
    return _GRAPHS[name]


def filter_plans(meta):
    pool, nb = meta["pool"], meta["nb"]
    n1 = meta["groups"][sg.T_N1]
    return {
        # the dropped constant is T_B-typed: it survives the type filter
        "filter-ne": Plan(T.PLANS["deg-ladder"].patterns, 2, [X, Y],
                          filters=[("ne", Y, int(pool[3]))]),
        "filter-or": Plan(T.PLANS["hub-nodrop"].patterns, 2, [X, Y],
                          filters=[("or", ("eq", X, int(n1[1])),
                                    ("eq", Y, int(nb[0])))]),
    }


def group_plans(meta):
    """The c2k (PM_LIST) shapes of group_graph as plain patterns, and a
    plan whose FIRST pattern starts from the constant."""
    c = int(meta["c_list"])
    return {
        "c2k": Plan([(gg.T_START[1025], TYPE, IN, X), (X, gg.P_OPT, OUT, Y),
                     (c, gg.P_LIST, OUT, Y)], 2, [X, Y]),
        "c2k-k2u": Plan([(gg.T_START[513], TYPE, IN, X),
                         (c, gg.P_LIST, OUT, X), (X, gg.P_OPT, OUT, Y)], 2,
                        [X, Y]),
        "c2u-k2u": Plan([(c, gg.P_LIST, OUT, X), (X, gg.P_OPT, OUT, Y)], 2,
                        [X, Y]),
    }


def chain_plans():
    """The multi-pattern plans of test_gpu_chain_fusion (no UNION, no
    OPTIONAL): every tail shape from 257 start rows, three from 2049,
    and the two capacity plans."""
    out = {"%s-n257" % k: p
           for k, p in CF.tail_plans(CF.p_type(257)).items()}
    out.update(CF.CAP_PLANS)
    big = CF.tail_plans(CF.p_type(2049))
    for k in ("tail", "tail-rev", "tail-len8+1"):
        out["%s-n2049" % k] = big[k]
    return out


# plans of gate_graph(): the P_HUB ones expand over the segment that
# crosses the gate on one rank, the P_DEG one over a segment that does not
GATE_PLANS = ["hub-ladder", "hub-nodrop", "hub-onedrop", "deg-ladder"]


def plan_names():
    """graph -> plan names, without building a graph (collection time)."""
    return {
        "edge": list(T.PLANS) + list(T.MISS_PLANS) + ["filter-ne", "filter-or"],
        "group": ["c2k", "c2k-k2u", "c2u-k2u"],
        "chain": list(chain_plans()),
        "gate": list(GATE_PLANS),
    }


_PLANS, _WANT = {}, {}


def plans_of(gname):
    if gname not in _PLANS:
        cx = graph(gname)
        if gname == "edge":
            d = {**T.PLANS, **T.MISS_PLANS, **filter_plans(cx.meta)}
        elif gname == "group":
            d = group_plans(cx.meta)
        elif gname == "gate":
            d = {k: T.PLANS[k] for k in GATE_PLANS}
        else:
            d = chain_plans()
        assert list(d) == plan_names()[gname]
        _PLANS[gname] = d
    return _PLANS[gname]


def want_of(gname, name):
    """Single-partition oracle rows of a plan, sorted, computed once."""
    key = (gname, name)
    if key not in _WANT:
        cx, plan = graph(gname), plans_of(gname)[name]
        if plan.filters:
            rows = filter_ref.expected(cx.ora, plan)
        else:
            rows = cx.ora.run_query(plan)
        rows = sort_rows(rows)
        rows.setflags(write=False)
        _WANT[key] = rows
    return _WANT[key]


_CPU_PARTS = {}


def cpu_parts(gname, W):
    key = (gname, W)
    if key not in _CPU_PARTS:
        _CPU_PARTS[key] = pl.PartSet(graph(gname).triples, W)
    return _CPU_PARTS[key]


# ---------------------------------------------------------------------
# per-rank step cases
# ---------------------------------------------------------------------
def owned_values(meta, W, r):
    """StepCase hook: the start values rank r owns, the operator's own
    keys first, padded with owned P_DEG filler subjects."""
    fill = meta["filler"][4:244]
    fill = fill[fill % W == r]

    def pick(vals):
        return np.concatenate([vals[vals % W == r], fill]).astype(np.uint32)
    return pick


_RANK_CASES = {}


def rank_cases(cx, W, r, op):
    """The row counts and widths of T.step_cases over owned starts."""
    key = (W, r, op)
    if key not in _RANK_CASES:
        pick = owned_values(cx.meta, W, r)
        widths = [c for c in NCOLS if c >= (2 if T.OPS[op][0] == "k2k" else 1)]
        cases = []
        for i, n in enumerate(ROWS):
            c = widths[i % len(widths)]
            cases.append(T.StepCase(cx, op, n, c, i % c, choose=pick))
        have = {(k.n, k.ncols) for k in cases}
        for c in widths:
            if (257, c) not in have:
                cases.append(T.StepCase(cx, op, 257, c, c - 1, choose=pick))
        _RANK_CASES[key] = cases
    return _RANK_CASES[key]


_BIG_CASES = {}


def big_case(cx, op):
    if op not in _BIG_CASES:
        W, r = BIG_W, BIG_RANK

        def pick(vals):
            return vals[vals % W == r]
        _BIG_CASES[op] = T.StepCase(cx, op, BIG, 2, 1, big=True, choose=pick)
    return _BIG_CASES[op]


def owner_cases(cx, op):
    """The unsplit mixed tables of the nsrv=1 module at 257 and 2049
    rows (every width at 257)."""
    return [c for c in T.step_cases(cx, op) if c.n in (257, 2049)]


def _oracle_step(ora, case):
    ex = OracleExecutor(ora, case.plan)
    ex.load(case.table, case.v2c, 0)
    ex.step()
    return ex.table()


# ---------------------------------------------------------------------
# CPU part
# ---------------------------------------------------------------------
SPECIAL = ("ladder", "fn", "rfn_s", "rfn_o", "chain")


def _special_vertices(meta):
    v = [int(x) for k in SPECIAL for x in meta[k]]
    v += [int(meta["pool"][0]), int(meta["pool"][4999]), int(meta["nb"][2]),
          meta["multi"], meta["bad"]]            # the hubs of the IN lists
    return v


@pytest.mark.parametrize("W", WS)
def test_store_integrity(W):
    """check() == 0 on every partition; the owner of a special vertex
    returns its full adjacency list, every other rank nothing."""
    cx = graph("edge")
    ps = cpu_parts("edge", W)
    for st in ps.stores:
        assert st.check() == 0
    none = np.empty(0, dtype=np.uint32)
    seen = 0
    for v in _special_vertices(cx.meta):
        for pid in (TYPE, P_DEG, P_HUB, P_FN, P_RFN, P_CHAIN):
            for d in (OUT, IN):
                if pid == TYPE and d == IN:
                    continue
                full = cx.adj.get((v, pid, d), none)
                seen += len(full) > 0
                for r in range(W):
                    want = full if v % W == r else none
                    assert np.array_equal(
                        ps.stores[r].get_triples(v, pid, d), want), \
                        (W, r, v, pid, d)
                    assert np.array_equal(
                        ps.oras[r].get_triples(v, pid, d), want), \
                        (W, r, v, pid, d)
    assert seen > 100


@pytest.mark.parametrize("W", WS)
def test_partition_local_conditions(W):
    """What the GPU cases rely on, from seg_stats (see the module
    docstring for the ranks found)."""
    cx = graph("edge")
    ps = cpu_parts("edge", W)
    full = wk.Store(cx.triples)
    local_fn = []
    for r, st in enumerate(ps.stores):
        for pid in (P_FN, P_RFN):
            for d in (OUT, IN):
                k, e = st.seg_stats(pid, d)
                fk, fe = full.seg_stats(pid, d)
                if k and k == e and fk != fe:
                    local_fn.append((W, r, pid, d))
    assert sorted(local_fn) == sorted(
        (W, r, pid, d) for r, pid, d in LOCAL_FN[W]), (W, local_fn)
    assert any(pid == P_RFN and d == OUT for _, _, pid, d in local_fn), W
    # both sides of the `edges / keys <= 32` gate of the type-fused CSR
    sides = set()
    for st in ps.stores:
        for pid in (P_DEG, P_HUB):
            k, e = st.seg_stats(pid, OUT)
            assert k > 0
            sides.add((pid, e // k <= 32))    # the engine's integer gate
    assert sides == {(P_DEG, True), (P_HUB, False)}, (W, sides)
    empty = [(r, pid, d) for r, st in enumerate(ps.stores)
             for pid in (P_CHAIN, P_RFN) for d in (OUT, IN)
             if st.seg_stats(pid, d) == (0, 0)]
    # W=2 and W=3 leave no P_CHAIN / P_RFN segment empty
    assert sorted(empty) == sorted(EMPTY_SEGS.get(W, [])), (W, empty)
    assert (W == EMPTY_SEG_W) == bool(empty)


def test_gate_graph_moves_one_rank_across_the_gate():
    """gate_graph(): (P_HUB, OUT) is at or below 32 edges per key on
    rank GATE_RANK of GATE_W partitions and above on the full store and
    on every other rank; P_DEG does not move; edge_graph() is a prefix."""
    cx, base = graph("gate"), graph("edge")
    assert np.array_equal(cx.triples[:len(base.triples)], base.triples)
    assert len(cx.triples) == len(base.triples) + 2 * sg.N_GATE
    assert (cx.meta["gate_s"] % sg.GATE_W == sg.GATE_RANK).all()
    assert cx.meta["gate_s"][0] > base.meta["max_id"]
    full = wk.Store(cx.triples)
    assert full.check() == 0
    k, e = full.seg_stats(P_HUB, OUT)
    assert e // k > 32
    ps = cpu_parts("gate", sg.GATE_W)
    below = []
    for r, st in enumerate(ps.stores):
        assert st.check() == 0
        k, e = st.seg_stats(P_HUB, OUT)
        if e // k <= 32:
            below.append(r)
        k, e = st.seg_stats(P_DEG, OUT)
        assert e // k <= 32
    assert below == [sg.GATE_RANK]
    # the rank under the gate keeps rows of the P_HUB plans
    ora = ps.oras[sg.GATE_RANK]
    assert len(ora.run_query(T.PLANS["hub-ladder"])) > 0


def local_fn_rank(W):
    """The rank on which (P_RFN, OUT) is functional, and one on which it
    holds a key with several edges."""
    ps = cpu_parts("edge", W)
    stats = [st.seg_stats(P_RFN, OUT) for st in ps.stores]
    fn = [r for r, (k, e) in enumerate(stats) if k and k == e]
    multi = [r for r, (k, e) in enumerate(stats) if k and k < e]
    return fn[0], multi[0]


@pytest.mark.parametrize("op", list(T.OPS))
@pytest.mark.parametrize("W", WS)
def test_rank_step_ref_vs_partition_oracle(W, op):
    """step_ref on the FULL adjacency equals the oracle executor over
    the rank's own partition when every start is owned."""
    cx = graph("edge")
    ps = cpu_parts("edge", W)
    nonempty = False
    for r in range(W):
        for case in rank_cases(cx, W, r, op):
            start = case.table[:, case.col]
            assert (start % W == r).all(), case.id
            got = sort_rows(_oracle_step(ps.oras[r], case))
            want = case.ref()
            assert got.shape == want.shape, (W, r, case.id, got.shape,
                                             want.shape)
            assert np.array_equal(got, want), (W, r, case.id)
            nonempty |= case.n >= 255 and len(want) > 0
    assert nonempty == (op != "k2c-rfn-none"), (W, op)


@pytest.mark.parametrize("W", WS)
def test_ladder_degrees_owned_once(W):
    cx = graph("edge")
    owners = {}
    for r in range(W):
        case = rank_cases(cx, W, r, "k2u-deg")[ROWS.index(2049)]
        for v in np.unique(case.table[:, case.col]).tolist():
            if v in cx.meta["ladder"]:
                owners.setdefault(v, []).append(r)
    assert sorted(owners) == sorted(cx.meta["ladder"].tolist())
    assert all(len(o) == 1 for o in owners.values())
    degs = sorted(len(cx.adj[(v, P_DEG, OUT)]) for v in owners)
    assert degs == sorted(cx.meta["ladder_degs"])


def test_big_case_ref_vs_partition_oracle():
    cx = graph("edge")
    ora = cpu_parts("edge", BIG_W).oras[BIG_RANK]
    for op in T.BIG_OPS:
        case = big_case(cx, op)
        assert case.n == BIG and (case.table[:, 1] % BIG_W == BIG_RANK).all()
        got = sort_rows(_oracle_step(ora, case))
        assert _same(got, case.ref()) and len(got) > 0, op


@pytest.mark.parametrize("op", list(T.OPS))
@pytest.mark.parametrize("W", WS)
def test_single_owner_oracle(W, op):
    """The unsplit table on every rank: the per-rank results add up to
    step_ref of the whole table, each row answered by its owner."""
    cx = graph("edge")
    ps = cpu_parts("edge", W)
    for case in owner_cases(cx, op):
        parts = [_oracle_step(o, case) for o in ps.oras]
        for r, t in enumerate(parts):
            assert len(t) == 0 or (t[:, case.col] % W == r).all(), \
                (W, r, case.id)
        got = sort_rows(pl._concat(parts, case.ref().shape[1]))
        assert _same(got, case.ref()), (W, case.id)


def _loop_cases():
    return [(g, n) for g, names in plan_names().items() for n in names]


@pytest.mark.parametrize("gname,name", _loop_cases(),
                         ids=["%s-%s" % c for c in _loop_cases()])
@pytest.mark.parametrize("W", WS)
def test_loopback_oracle(W, gname, name):
    """The loopback driver over oracle executors equals the oracle of
    the unpartitioned graph."""
    plan = plans_of(gname)[name]
    want = want_of(gname, name)
    ps = cpu_parts(gname, W)
    trace = {}
    got = sort_rows(pl.run_plan(ps.oracle_executors(plan), plan, "host",
                                trace))
    assert _same(got, want), (W, gname, name, got.shape, want.shape)
    if name not in ("tail-eq-none-n257", "tail-fn-outside-n257",
                    "tail-type-outside-n257"):
        assert len(want) > 0, name
    if name.startswith("c2k"):
        assert trace["list_filters"] == 1


def test_routing_moves_rows():
    """With re-splitting disabled the type filter of `deg-ladder` probes
    the new column on the rank that expanded it, not on its owner: rows
    are lost."""
    plan, want = plans_of("edge")["deg-ladder"], want_of("edge", "deg-ladder")
    ps = cpu_parts("edge", 3)
    trace = {}
    got = sort_rows(pl.run_plan(ps.oracle_executors(plan), plan, "host",
                                trace))
    assert _same(got, want) and trace["moved"] > 0
    bad = sort_rows(pl.run_plan(ps.oracle_executors(plan), plan, None))
    assert not _same(bad, want)
    assert 0 < len(bad) < len(want)


# ---------------------------------------------------------------------
# filter-list cases
# ---------------------------------------------------------------------
LIST_LENS = [0, 1, 2, 63, 64, 65, 1025]
LIST_ROWS = [0, 1, 255, 256, 257, 1025, 2049]


def flist(L):
    """A sorted list of L ids with a gap between any two members."""
    return (B + 10 + 3 * np.arange(L)).astype(np.uint32)


def flist_probes(lst):
    """first, last, one below the first, one above the last, an absent
    value between two members; other absent values around them."""
    if len(lst) == 0:
        return np.array([B, B + 10, 5, 0xFFFFFFFE], dtype=np.uint32)
    p = [lst[0], lst[-1], lst[0] - 1, lst[-1] + 1, 5, B]
    if len(lst) > 1:
        p += [lst[0] + 1, lst[len(lst) // 2] + 1, lst[-1] - 1,
              lst[len(lst) // 2]]
    return np.array(p, dtype=np.uint32)


def flist_table(lst, n, ncols, col):
    r = np.arange(n, dtype=np.int64)
    t = np.empty((n, ncols), dtype=np.uint32)
    for j in range(ncols):
        t[:, j] = B + (r * (j + 3) + j) % 1000
    probes = flist_probes(lst)
    # every probe, then members and near misses over the whole list
    walk = (B + 10 + (r * 7) % (3 * max(len(lst), 1) + 6)).astype(np.uint32)
    vals = np.concatenate([probes, walk])[:n] if n else walk[:0]
    t[:, col] = np.resize(vals, n) if n else vals
    return t


def test_filter_list_inputs():
    """The numpy side of the list cases: every probe class occurs."""
    for L in LIST_LENS:
        lst = flist(L)
        assert len(lst) == L and (np.diff(lst.astype(np.int64)) > 1).all()
        t = flist_table(lst, 2049, 4, 3)
        hit = np.isin(t[:, 3], lst)
        assert hit.any() == (L > 0) and not hit.all()
        if L:
            assert np.isin(flist_probes(lst)[:2], lst).all()
            assert not np.isin(flist_probes(lst)[2:6], lst).any()
        if L > 1:
            p = flist_probes(lst)
            assert not np.isin(p[6:9], lst).any() and p[9] in lst


# ---------------------------------------------------------------------
# GPU part
# ---------------------------------------------------------------------
_LIVE = {"key": None, "ps": None}


def _drop_live():
    if _LIVE["ps"] is not None:
        _LIVE["ps"].close()
    _LIVE["key"], _LIVE["ps"] = None, None
    gc.collect()


def live_parts(gname, W, config):
    """The one PartSet with engines alive at a time (at most 8 engines):
    asking for another one drops the current one first."""
    key = (gname, W, config)
    if _LIVE["key"] != key:
        _drop_live()
        ps = pl.PartSet(graph(gname).triples, W, STORE_ENVS[config])
        ps.build_engines(device=0, **TIMED)
        _LIVE["key"], _LIVE["ps"] = key, ps
    return _LIVE["ps"]


@pytest.fixture(scope="module", autouse=True)
def _release_engines():
    yield
    _drop_live()


def _launches(eng):
    return {k: v["launches"] for k, v in eng.kernel_stats().items()}


def _delta(eng, before):
    now = _launches(eng)
    return {k: now[k] - before[k] for k in now}


def _run_step(eng, case):
    eng.begin_query(case.plan)
    eng.load_rbuf(case.table, case.v2c, 0)
    n = eng.execute_one_pattern()
    got = eng.fetch_raw()
    assert n == got.shape[0], (case.id, n, got.shape)
    return got


def _part_id(p):
    return "%d-%s" % p


@pytest.mark.gpu
@pytest.mark.parametrize("op", list(T.OPS))
@pytest.mark.parametrize("part", PARTS, ids=_part_id)
def test_partition_step_operator(part, op):
    """One step of every operator on every rank, over the starts that
    rank owns, against step_ref on the full adjacency: the per-partition
    functional maps, CSR index, type_of / type bitmaps and cluster hash
    at the row counts and widths of the nsrv=1 module; the multi-tile
    scan carry (BIG_OPS) on one rank of W=3."""
    W, config = part
    cx = graph("edge")
    ps = live_parts("edge", W, config)
    for r, eng in enumerate(ps.engines):
        cases = list(rank_cases(cx, W, r, op))
        if W == BIG_W and r == BIG_RANK and op in T.BIG_OPS:
            cases.append(big_case(cx, op))
        for case in cases:
            got = _run_step(eng, case)
            want = case.ref()
            assert got.shape == want.shape, (W, r, case.id, got.shape,
                                             want.shape)
            assert np.array_equal(sort_rows(got), want), (W, r, case.id)


@pytest.mark.gpu
@pytest.mark.parametrize("op", list(T.OPS))
@pytest.mark.parametrize("W", WS)
def test_single_owner(W, op):
    """The unsplit mixed table of the nsrv=1 case, unchanged, on every
    rank: no side index answers for a key it does not own and none drops
    a key it owns, so the ranks' results add up to step_ref of the whole
    table."""
    cx = graph("edge")
    ps = live_parts("edge", W, "default")
    for case in owner_cases(cx, op):
        parts = [_run_step(eng, case) for eng in ps.engines]
        for r, t in enumerate(parts):
            assert len(t) == 0 or (t[:, case.col] % W == r).all(), \
                (W, r, case.id)
        got = sort_rows(pl._concat(parts, case.ref().shape[1]))
        assert _same(got, case.ref()), (W, case.id)


def _plan_params():
    out, ids = [], []
    for W, config in PARTS:
        for gname, names in plan_names().items():
            for exch in ("host", "device"):
                for name in names:
                    out.append((W, config, gname, exch, name))
                    ids.append("%d-%s-%s-%s%s" % (
                        W, config, exch, "gate-" if gname == "gate" else "",
                        name))
    # one live PartSet per (graph, W, config): keep its cases together
    order = sorted(range(len(out)), key=lambda i: (
        PARTS.index(out[i][:2]), list(plan_names()).index(out[i][2])))
    return [out[i] for i in order], [ids[i] for i in order]


@pytest.mark.gpu
@pytest.mark.parametrize("W,config,gname,exch,name", _plan_params()[0],
                         ids=_plan_params()[1])
def test_partition_plans(W, config, gname, exch, name):
    """The loopback with one engine per rank, rows moved through the
    host and through generate_sub_query + load_rbuf_device, against the
    oracle of the unpartitioned graph.  The loopback drives the step
    API, one launch chain per pattern: the chain fusion and its
    reversed-map forms need a whole-plan run and are reached by
    test_partition_local_chain_plans, not here."""
    plan = plans_of(gname)[name]
    want = want_of(gname, name)
    ps = live_parts(gname, W, config)
    before = [_launches(e) for e in ps.engines]
    trace = {}
    got = sort_rows(pl.run_plan(ps.engine_executors(plan), plan, exch, trace))
    assert _same(got, want), (W, config, gname, exch, name, got.shape,
                              want.shape)
    d = [_delta(e, b) for e, b in zip(ps.engines, before)]
    if exch == "device" and trace["moved"]:
        assert sum(x["split"] for x in d) > 0, (name, d)
    if trace["list_filters"]:
        # execute_filter_list ran on every rank
        assert all(x["filter"] >= trace["list_filters"] for x in d), (name, d)


def _check_filter_list(eng, what):
    pid = P_DEG
    const = int(B + 1)
    for L in LIST_LENS:
        lst = flist(L)
        for n in LIST_ROWS:
            for ncols in (1, 4, 7):
                for col in sorted({0, ncols - 1}):
                    t = flist_table(lst, n, ncols, col)
                    plan = Plan([(const, pid, OUT, -(col + 1))], nvars=ncols,
                                required_vars=[-1])
                    eng.begin_query(plan)
                    eng.load_rbuf(t, list(range(ncols)), 0)
                    before = _launches(eng)
                    cnt = eng.execute_filter_list(lst)
                    assert _delta(eng, before)["filter"] == 1
                    got = eng.fetch_raw().reshape(-1, ncols)
                    want = t[np.isin(t[:, col], lst)]
                    assert cnt == len(want) == len(got), \
                        (what, L, n, ncols, col, cnt, len(want))
                    assert _same(sort_rows(got), sort_rows(want)), \
                        (what, L, n, ncols, col)
                    assert eng.pattern_step == 1
    # refusals: a variable subject, an object without a column
    t = flist_table(flist(64), 257, 2, 1)
    for pat, v2c in (((-1, pid, OUT, -2), [0, 1]),
                     ((const, pid, OUT, -3), [0, 1, -1])):
        eng.begin_query(Plan([pat], nvars=len(v2c), required_vars=[-1]))
        eng.load_rbuf(t, v2c, 0)
        with pytest.raises(RuntimeError, match="rc=-3"):     # WK_ERR_PLAN
            eng.execute_filter_list(flist(64))
    # still exact afterwards
    eng.begin_query(Plan([(const, pid, OUT, -2)], nvars=2, required_vars=[-1]))
    eng.load_rbuf(t, [0, 1], 0)
    assert eng.execute_filter_list(flist(64)) == \
        int(np.isin(t[:, 1], flist(64)).sum())


@pytest.mark.gpu
def test_filter_list_edges():
    """execute_filter_list (PM_LIST against a caller-supplied list)
    against numpy.isin on an nsrv=1 engine and on a rank of W=3: list
    lengths around the binary search's steps, probes on and next to both
    ends of the list, tables around the 256-row tile, first and last
    column of 1, 4 and 7."""
    cx = graph("edge")
    _drop_live()          # the nsrv=1 engine must not be a ninth one
    with env(**TIMED):
        eng = wk.Engine(wk.Store(cx.triples), device=0)
    _check_filter_list(eng, "nsrv=1")
    del eng
    gc.collect()
    ps = live_parts("edge", 3, "default")
    _check_filter_list(ps.engines[1], "W=3 rank 1")


# ---- whole-plan entry points on one partition ------------------------
ENTRIES = ["run_query", "submit", "graph", "plan_batch", "light2",
           "light_batch"]
# overflow entries of the LDS plan interpreter on the unpartitioned
# store (test_plan_batch_capacity_boundary): template -> const indexes
LP_OVF_FULL = {"one": {2}, "two": {1}, "typed": {3}}


def lp_overflows(ora, tmpl, const):
    """Whether the interpreter's table outgrows its LP_CAP slots on the
    store `ora` restates: the first list has more than LP_CAP entries,
    or an expansion leaves rows * columns above LP_CAP (a filter only
    shrinks the table)."""
    rows = ora.get_triples(int(const), tmpl.patterns[0][1], OUT)
    if len(rows) > LP_CAP:
        return True
    ncols = 1
    for s, p, d, o in tmpl.patterns[1:]:
        if o < 0 and p != TYPE:          # the k2u of the `two` template
            rows = np.concatenate([ora.get_triples(int(v), p, d)
                                   for v in rows] + [rows[:0]])
            ncols += 1
            if len(rows) * ncols > LP_CAP:
                return True
    return False


def test_lp_overflow_rule_on_full_store():
    """The rule reproduces the overflow entries pinned for nsrv=1."""
    cx = graph("edge")
    for name, (tmpl, consts) in T._lp_plans(cx.meta).items():
        got = {k for k, c in enumerate(consts)
               if lp_overflows(cx.ora, tmpl, c)}
        assert got == LP_OVF_FULL[name], (name, got)


def _via(eng, plan, entry):
    """Rows (sorted) of `plan` through one entry point."""
    if entry == "run_query":
        return sort_rows(eng.run_query(plan))
    eng.submit(plan)
    return sort_rows(eng.fetch_result())


def _whole_plans_edge(cx):
    d = {**T.PLANS, **T.MISS_PLANS}
    for name, (tmpl, consts) in T._lp_plans(cx.meta).items():
        for k, c in enumerate(consts):
            d["lp-%s-%d" % (name, k)] = T._with_const(tmpl, c)
    return d


def _light_plan(const, cval):
    return Plan([(int(const), gg.P_L, OUT, X), (X, TYPE, OUT, cval)], nvars=1,
                required_vars=[X])


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("W", WS)
def test_partition_local_whole_plan(W, entry):
    """A whole-plan entry point on partition r returns what the oracle
    restatement returns on the same partition,
    OracleCtx(triples, sid=r, nsrv=W).run_query(plan): the type filter
    runs on a column whose values the partition mostly does not own, and
    keeps the owned ones only."""
    gname = "light" if entry.startswith("light") else "edge"
    cx = graph(gname)
    ps = live_parts(gname, W, "default")
    total = novf = 0
    for r, (eng, ora) in enumerate(zip(ps.engines, ps.oras)):
        if entry in ("run_query", "submit"):
            for name, plan in _whole_plans_edge(cx).items():
                want = sort_rows(ora.run_query(plan))
                got = _via(eng, plan, entry)
                assert _same(got, want), (W, r, entry, name, got.shape,
                                          want.shape)
                total += len(want)
        elif entry == "graph":
            for name, plan in {**T.PLANS, **T.MISS_PLANS}.items():
                want = sort_rows(ora.run_query(plan))
                gid = eng.graph_build(plan)
                for _ in range(2):
                    # a store with type bitmaps replays exactly
                    assert eng.graph_run(gid) == len(want), (W, r, name)
                    assert _same(_via(eng, plan, "run_query"), want), \
                        (W, r, name, "plain path after the replay")
                total += len(want)
        elif entry == "plan_batch":
            ovf = np.uint64(wk.LP_OVERFLOW)
            for name, (tmpl, consts) in T._lp_plans(cx.meta).items():
                eng.submit_plan_batch(tmpl, consts)
                got = eng.wait_light_batch()
                for k, (c, n) in enumerate(zip(consts, got)):
                    if lp_overflows(ora, tmpl, c):
                        assert n == ovf and c % W == r, (W, r, name, k)
                        novf += 1
                        continue
                    want = len(ora.run_query(T._with_const(tmpl, c)))
                    assert n == want, (W, r, name, k, int(n), want)
                    total += want
        elif entry == "light2":
            for c in list(cx.meta["consts"]) + [cx.meta["absent"]]:
                for cval in (gg.LT_F, gg.LT_O):
                    plan = _light_plan(c, cval)
                    want = sort_rows(ora.run_query(plan))
                    for e2 in ("submit", "run_query"):
                        got = _via(eng, plan, e2)
                        assert _same(got, want), (W, r, int(c), cval, e2)
                    total += len(want)
        else:
            subj = [int(c) for c in cx.meta["consts"]] + [cx.meta["absent"]]
            for cval in (gg.LT_F, gg.LT_O):
                n = len(subj)
                eng.submit_light_batch(subj, [gg.P_L] * n, [OUT] * n,
                                       [cval] * n)
                got = eng.wait_light_batch()
                want = [len(ora.run_query(_light_plan(c, cval)))
                        for c in subj]
                assert got.tolist() == want, (W, r, cval)
                total += sum(want)
    assert total > 0, (W, entry)          # some rank owns and keeps rows
    if entry == "plan_batch":
        # the two single-list overflows, each on its constant's owner
        assert novf >= 2, (W, novf)


CHAIN_ENTRIES = ["run_query", "submit", "graph"]


@pytest.mark.gpu
@pytest.mark.parametrize("entry", CHAIN_ENTRIES)
@pytest.mark.parametrize("W", WS)
def test_partition_local_chain_plans(W, entry):
    """The chain-fusion plans as WHOLE plans on every partition of the
    chain graph against the oracle restatement on the same partition.
    Only a whole-plan run considers the chain fusion, the type-fused CSR
    pipeline and the reversed functional map behind them (tail-rev,
    tail-eq, tail-len8+1), all of which are complete on a
    single-partition store only: taken on a partition they would lose
    the rows whose other endpoint another rank owns."""
    cx = graph("chain")
    ps = live_parts("chain", W, "default")
    total = 0
    for r, (eng, ora) in enumerate(zip(ps.engines, ps.oras)):
        for name, plan in chain_plans().items():
            want = sort_rows(ora.run_query(plan))
            if entry == "graph":
                gid = eng.graph_build(plan)
                for _ in range(2):
                    assert eng.graph_run(gid) == len(want), (W, r, name)
                got = sort_rows(eng.fetch_result(plan))
            else:
                got = _via(eng, plan, entry)
            assert _same(got, want), (W, r, entry, name, got.shape,
                                      want.shape)
            total += len(want)
    assert total > 0, (W, entry)


def test_chain_plans_partition_oracle_not_vacuous():
    """For W=3 the reversed-map and chain plans keep rows on a
    partition, and fewer than on the full store: a run that took a
    single-partition path would not go unnoticed.  (With W=2 and W=8
    the ids of the chain graph put a student and its department on
    different ranks, so most of these plans are empty there.)"""
    oras = cpu_parts("chain", 3).oras
    for name in ("tail-rev-n2049", "tail-len8+1-n2049", "tail-n2049",
                 "tail-rev-n257", "tail-eq-n257", "tail-len5-n257",
                 "tail-all-n257", "cap-members", "cap-ladder"):
        plan = chain_plans()[name]
        per = [len(o.run_query(plan)) for o in oras]
        assert 0 < sum(per) < len(want_of("chain", name)), (name, per)


@pytest.mark.gpu
@pytest.mark.parametrize("W", WS)
def test_partition_local_functional_launch(W):
    """(P_RFN, OUT) is functional on one rank only: a k2u step over its
    owned keys runs an expand launch there and is exact; the rank where
    the segment holds a multi-edge key is exact too."""
    cx = graph("edge")
    ps = live_parts("edge", W, "default")
    fn_rank, multi_rank = local_fn_rank(W)
    assert (W, fn_rank, P_RFN, OUT) in [(W,) + x for x in LOCAL_FN[W]]
    for r in (fn_rank, multi_rank):
        vals = np.array([v for v in cx.meta["rfn_s"].tolist() +
                         cx.meta["ladder"].tolist() if v % W == r],
                        dtype=np.uint32)
        eng = ps.engines[r]
        for n in (1, 257, 2049):
            t = np.stack([np.resize(vals, n),
                          (B + np.arange(n) % 997).astype(np.uint32)], axis=1)
            plan = Plan([(X, P_RFN, OUT, -3)], nvars=3, required_vars=[X])
            eng.begin_query(plan)
            eng.load_rbuf(t, [0, 1, -1], 0)
            before = _launches(eng)
            cnt = eng.execute_one_pattern()
            assert _delta(eng, before)["expand"] >= 1, (W, r, n)
            want = sort_rows(step_ref(t, 0, cx.adj, "k2u", P_RFN, OUT))
            got = eng.fetch_raw()
            assert cnt == len(want) > 0, (W, r, n)
            assert _same(sort_rows(got), want), (W, r, n)
            # one edge per owned key on the functional rank, more on the other
            nkeys = int(np.isin(t[:, 0], cx.meta["rfn_s"]).sum())
            assert (cnt == nkeys) == (r == fn_rank), (W, r, n, cnt, nkeys)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", CHAIN_ENTRIES)
def test_partition_local_gate_plans(entry):
    """gate_graph() on GATE_W partitions: one rank sees (P_HUB, OUT) on
    the other side of the `edges / keys <= 32` gate than the full store.
    Whole plans on every rank equal the partition oracle, and a P_HUB
    k2u step over the keys that rank owns equals step_ref."""
    W = sg.GATE_W
    cx = graph("gate")
    ps = live_parts("gate", W, "default")
    total = {}
    for r, (eng, ora) in enumerate(zip(ps.engines, ps.oras)):
        for name in GATE_PLANS:
            plan = T.PLANS[name]
            want = sort_rows(ora.run_query(plan))
            if entry == "graph":
                gid = eng.graph_build(plan)
                for _ in range(2):
                    assert eng.graph_run(gid) == len(want), (r, name)
                got = sort_rows(eng.fetch_result(plan))
            else:
                got = _via(eng, plan, entry)
            assert _same(got, want), (r, entry, name, got.shape, want.shape)
            total[r] = total.get(r, 0) + len(want)
    assert total[sg.GATE_RANK] > 0
    r = sg.GATE_RANK
    vals = np.array([v for v in cx.meta["gate_s"].tolist() +
                     cx.meta["ladder"].tolist() if v % W == r],
                    dtype=np.uint32)
    for n in (1, 257, 2049):
        t = np.resize(vals, n)[:, None]
        plan = Plan([(X, P_HUB, OUT, Y)], nvars=2, required_vars=[X])
        eng = ps.engines[r]
        eng.begin_query(plan)
        eng.load_rbuf(t, [0, -1], 0)
        cnt = eng.execute_one_pattern()
        want = sort_rows(step_ref(t, 0, cx.adj, "k2u", P_HUB, OUT))
        assert cnt == len(want) > 0
        assert _same(sort_rows(eng.fetch_raw()), want), n
