"""Edge tests for the LDS plan interpreter (k_plan_batch, compiled by
compile_light_plan, entered through wk_engine_submit_plan_batch) on the
synthetic graph of lp_graph.py.

The interpreter returns counts only.  The CPU part therefore proves,
without a GPU, that the counts can tell a wrong kernel from a right one:
lp_ref equals the oracle restatement and the brute-force evaluator for
every template and constant, the graph holds every condition it was
built for, the deliberately wrong variants (wrong subject column,
swapped k2k columns, a row stride one column short) give other counts,
and exactly the intended boundary cases overflow.  The GPU part compares
the engine with lp_ref alone, by integer equality.
"""
import gc

import numpy as np
import pytest

import wukong_amd as wk
from wukong_amd import Plan
from tests import lp_graph as lg
from tests import oracle_util
from tests import part_loop as pl
from tests import synth_graph as sg
from tests.oracle_util import OracleCtx
from tests.lp_graph import (P_A, P_B, P_C, P_D, P_U, P_H, P_K, P_N, P_E, P_F,
                            P_G, P_NONE, P_PAST, T_X, T_Y, T_M, X, Y, Z,
                            lp_ref)
from tests.synth_graph import B, IN, OUT, TYPE, LP_CAP

OVF = np.uint64(wk.LP_OVERFLOW)
PART_W = 3


def plan_of(pats, nvars, const=None, **kw):
    pats = list(pats)
    if const is not None:
        pats[0] = (int(const),) + tuple(pats[0][1:])
    return Plan(pats, nvars, list(range(-1, -nvars - 1, -1)), **kw)


class Ctx:
    """One variant of the graph, its adjacency, templates and the
    reference (count, overflows) of every (template, constant), computed
    once and left unchanged."""

    def __init__(self, multi):
        self.triples, self.meta = lg.lp_graph(multi)
        self.adj = sg.adjacency(self.triples)
        self.tmpl = lg.templates(self.meta)
        self.ref = {(name, k): lp_ref(self.adj, pats, c)
                    for name, (pats, nv, consts) in self.tmpl.items()
                    for k, c in enumerate(consts)}

    def template(self, name):
        pats, nv, consts = self.tmpl[name]
        return plan_of(pats, nv, consts[0]), [int(c) for c in consts]

    def plan(self, name, k):
        pats, nv, consts = self.tmpl[name]
        return plan_of(pats, nv, consts[k])

    def want(self, name):
        """Expected counts array of a template's own window."""
        n = len(self.tmpl[name][2])
        return [OVF if self.ref[name, k][1] else self.ref[name, k][0]
                for k in range(n)]


def fit_rows(cx, name):
    """Rows the unpartitioned graph keeps in the template's entries that
    fit: where there are some, some rank has to keep some."""
    return sum(n for (t, k), (n, ovf) in cx.ref.items()
               if t == name and not ovf)


_CTX = {}


def get_ctx(variant):
    if variant not in _CTX:
        _CTX[variant] = Ctx(variant == "multi")
    return _CTX[variant]


VARIANTS = ["single", "multi"]
NAMES = list(lg.templates(lg.lp_graph(False)[1]))


@pytest.fixture(scope="module", params=VARIANTS)
def ctx(request):
    return get_ctx(request.param)


# ---------------------------------------------------------------------
# CPU part
# ---------------------------------------------------------------------
def test_ref_vs_oracle_vs_brute(ctx):
    ora = OracleCtx(ctx.triples)
    for name, (pats, nv, consts) in ctx.tmpl.items():
        for k, c in enumerate(consts):
            plan = ctx.plan(name, k)
            n = ctx.ref[name, k][0]
            assert n == len(ora.run_query(plan)), (name, k)
            assert n == len(ora.brute_query(plan)), (name, k)


def test_ref_vs_partition_oracle(ctx):
    """lp_ref on the lists a rank owns == the oracle restatement of that
    partition; every template keeps rows on some rank."""
    kept = {name: 0 for name in ctx.tmpl}
    for r in range(PART_W):
        ora = OracleCtx(ctx.triples, sid=r, nsrv=PART_W)
        adj = lg.owned(ctx.adj, r, PART_W)
        for name, (pats, nv, consts) in ctx.tmpl.items():
            for k, c in enumerate(consts):
                n = lp_ref(adj, pats, c)[0]
                assert n == len(ora.run_query(ctx.plan(name, k))), (r, name, k)
                kept[name] += n
    for name in ctx.tmpl:
        assert (kept[name] > 0) == (fit_rows(ctx, name) > 0), name


def test_store_and_variants(ctx):
    meta = ctx.meta
    assert 1000 <= len(ctx.triples) <= 50000
    assert int(ctx.triples[:, [0, 2]].max()) == meta["last_v"]
    store = wk.Store(ctx.triples)
    assert store.check() == 0
    for key, want in ctx.adj.items():
        if key[1] in (P_K, P_N, P_H, P_D, TYPE):
            assert np.array_equal(store.get_triples(*key), want), key
    ntypes = {}
    for s, p, o in np.unique(ctx.triples, axis=0).tolist():
        if p == TYPE:
            ntypes[s] = ntypes.get(s, 0) + 1
    two = [s for s, n in ntypes.items() if n > 1]
    assert two == ([meta["multi_v"]] if meta["multi"] else [])
    # the variants differ by that one triple only
    other = get_ctx("single" if meta["multi"] else "multi")
    assert abs(len(ctx.triples) - len(other.triples)) == 1


def test_row_counts_around_the_wave(ctx):
    meta = ctx.meta
    consts = lg.rc_consts(meta)
    sizes = [len(ctx.adj.get((c, P_A, OUT), [])) for c in consts]
    assert sizes == [0, 0, 1, 63, 64, 65, 129]
    vids = set(ctx.triples[:, [0, 2]].ravel().tolist())
    assert meta["nokey"] in vids and meta["absent"] not in vids
    # every op kind is entered with each of these sizes: the functional
    # P_U keeps the row count on the way to a two-column table
    mid = meta["mid"]
    assert all(len(ctx.adj[int(m), P_U, OUT]) == 1 for m in mid)
    entered = {"c2u": 0, "k2u-last": 1, "k2u-col0": 1, "k2u-in": 2,
               "k2k-lr": 2, "k2k-rl": 2, "k2c-1col": 1, "type-1col": 1}
    for name, nops in entered.items():
        pats, nv, cs = ctx.tmpl[name]
        assert cs == consts, name
        got = [lp_ref(ctx.adj, pats[:max(nops, 1)], c)[0] for c in cs]
        assert got == sizes, name
    for name in ("k2c-3col", "type-inner"):
        assert ctx.tmpl[name][2] == consts


def test_k2u_conditions(ctx):
    adj, mid = ctx.adj, ctx.meta["mid"]
    db = [len(adj[int(m), P_B, OUT]) for m in mid]
    dc = [len(adj[int(m), P_C, OUT]) for m in mid]
    assert any(a != b for a, b in zip(db[:63], dc[:63]))
    assert sum(db[:63]) != sum(dc[:63])
    pats = ctx.tmpl["k2u-col0"][0]
    assert pats[2][0] == X and len(pats) == 3      # column 0 of 2 columns
    pats = ctx.tmpl["k2u-in"][0]
    assert pats[2][:3] == (X, P_D, IN)
    have = [(int(m), P_D, IN) in adj for m in mid[:63]]
    assert any(have) and not all(have) and not have[3]
    assert {len(adj.get((int(m), P_D, IN), [])) for m in mid[:63]} == {0, 1, 2}


def test_k2k_conditions(ctx):
    adj, meta = ctx.adj, ctx.meta
    seen = set()
    nolist = 0
    for i, m in enumerate(meta["mid"][:63]):     # all inside the 63-row case
        u = int(adj[int(m), P_U, OUT][0])
        lst = adj.get((int(m), P_K, OUT))
        if lst is None:
            nolist += 1
            continue
        assert len(lst) == lg.k_len(i)
        where = ("first" if lst[0] == u else "last" if lst[-1] == u
                 else "absent")
        if len(lst) > 1:
            assert where == lg.k_mode(i), i
            assert (u in lst.tolist()) == (where != "absent")
        if where == "absent" and len(lst) > 1:
            assert lst[0] < u < lst[-1]            # the search runs to the end
        seen.add((len(lst), where))
    assert nolist >= 1
    for L in lg.K_LENS:
        want = {"first", "last", "absent"} if L > 1 else {"first", "absent"}
        assert {w for n, w in seen if n == L} == want, L
    # subject column left of the object column, and right of it
    lr, rl = ctx.tmpl["k2k-lr"][0][2], ctx.tmpl["k2k-rl"][0][2]
    assert (lr[0], lr[3]) == (X, Y) and (rl[0], rl[3]) == (Y, X)


def test_k2c_conditions(ctx):
    adj, meta = ctx.adj, ctx.meta
    c = meta["nconst"]
    classes = set()
    for m in meta["mid"][:63]:
        lst = adj.get((int(m), P_N, OUT))
        if lst is None:
            classes.add("nolist")
        elif lst[0] == c:
            classes.add("first")
        elif lst[-1] == c:
            classes.add("last")
        elif c < lst[0]:
            classes.add("below")
        elif c > lst[-1]:
            classes.add("above")
        else:
            assert c not in lst.tolist()
            classes.add("absent")
    assert classes == {"nolist", "first", "last", "below", "above", "absent"}
    pats, nv, _ = ctx.tmpl["k2c-3col"]
    assert pats[3][0] == X and pats[3][1] == P_N and nv == 3


def test_type_column_conditions(ctx):
    adj, meta = ctx.adj, ctx.meta
    pats, nv, consts = ctx.tmpl["type-inner"]
    assert nv == 3 and pats[3][:3] == (Y, TYPE, OUT)   # the inner column
    col = set()
    for m in meta["mid"][:63]:
        col |= set(adj[int(m), P_B, OUT].tolist())
    assert meta["last_v"] in col and meta["low_v"] in col
    assert meta["low_v"] < B <= min(v for v in col if v != meta["low_v"])
    assert meta["multi_v"] in col
    assert any((v, TYPE, OUT) not in adj for v in col if v >= B)
    # the 1-row case already reads the last vid of the graph
    assert meta["last_v"] in adj[int(meta["mid"][0]), P_B, OUT].tolist()
    assert adj[meta["last_v"], TYPE, OUT].tolist() == [T_X]
    # the second type changes the count
    a = get_ctx("single").ref["type-inner", 3][0]
    b = get_ctx("multi").ref["type-inner", 3][0]
    assert b == a + sum(meta["multi_v"] in adj[int(m), P_B, OUT].tolist()
                        for m in meta["mid"][:63]) * 1 and b > a


def test_chain_collisions(ctx):
    """22 P_H keys in one bucket of 8 walk three chained buckets, 16 in
    another walk two; chain_miss hashes to the long bucket and is no
    key.  Buckets are recomputed with the oracle's own hash."""
    meta = ctx.meta
    chain = meta["chain"]
    store = wk.Store(ctx.triples)
    k, _ = store.seg_stats(P_H, OUT)
    assert k == sg.N_CHAIN == len(chain) and (k + 4) // 5 == sg.CHAIN_BUCKETS
    occ = np.zeros(sg.CHAIN_BUCKETS, dtype=int)
    for v in chain:
        key = oracle_util.key_pack(int(v), P_H, OUT)
        assert key == wk.key_pack(int(v), P_H, OUT)
        occ[oracle_util.hash_u64(key) % sg.CHAIN_BUCKETS] += 1
    assert occ[meta["chain_long_bucket"]] == sg.CHAIN_LONG > 3 * 7
    assert 2 * 7 < occ[meta["chain_mid_bucket"]] == sg.CHAIN_MID <= 3 * 7
    miss = meta["chain_miss"]
    assert miss not in chain.tolist() and (miss, P_H, OUT) not in ctx.adj
    assert oracle_util.hash_u64(oracle_util.key_pack(miss, P_H, OUT)) \
        % sg.CHAIN_BUCKETS == meta["chain_long_bucket"]
    # the probed column holds all of them, mid-plan
    col = ctx.adj[meta["r_chain"], P_A, OUT].tolist()
    assert set(col) == set(chain.tolist()) | {miss}
    for name in ("chain-k2u", "chain-k2k", "chain-k2c"):
        assert 0 < ctx.ref[name, 0][0]
    assert ctx.ref["chain-k2k", 0][0] < ctx.ref["chain-k2u", 0][0]


def test_empty_segments(ctx):
    store = wk.Store(ctx.triples)
    assert store.seg_stats(TYPE, OUT)[0] > 0
    for pid, d in ((P_NONE, OUT), (P_NONE, IN), (P_PAST, OUT), (P_PAST, IN)):
        assert not any(k[1] == pid for k in ctx.adj)
    assert not any(k[1] == TYPE and k[2] == IN for k in ctx.adj)
    assert P_NONE < int(ctx.triples[:, 1].max()) < P_PAST
    for op in ("c2u", "k2u", "k2k", "k2c"):
        for fam in ("tin", "none"):
            name = "%s-%s" % (fam, op)
            assert all(ctx.ref[name, k] == (0, False)
                       for k in range(len(ctx.tmpl[name][2]))), name
    # the tables that enter those ops are not empty
    assert ctx.ref["k2u-in", 5][0] > 0 and ctx.ref["c2u", 5][0] == 65


def test_emptied_table(ctx):
    pats, nv, consts = ctx.tmpl["emptied"]
    for k, c in enumerate(consts):
        assert lp_ref(ctx.adj, pats[:1], c)[0] > 0
        assert lp_ref(ctx.adj, pats[:2], c)[0] == 0       # the filter
        assert lp_ref(ctx.adj, [pats[0]] + pats[2:], c)[0] > 0
        assert ctx.ref["emptied", k] == (0, False)
    kinds = [(p[3] < 0, p[3]) for p in pats[2:]]
    assert kinds == [(True, Y), (True, Y)]        # a k2u, then a k2k


def test_capacity_boundaries(ctx):
    adj, meta = ctx.adj, ctx.meta
    assert lg.ROWS3 * 3 == LP_CAP == lg.ROWS4 * 4
    assert (lg.ROWS3, lg.ROWS4) == (2048, 1536)
    assert max(len(v) for v in adj.values()) <= LP_CAP // 4
    assert ctx.ref["cap3", 0] == (lg.ROWS3, False)
    assert ctx.ref["cap3", 1] == (lg.ROWS3 + 1, True)
    assert ctx.ref["cap4", 0] == (lg.ROWS4, False)
    assert ctx.ref["cap4", 1] == (lg.ROWS4 + 1, True)
    # the step before the last still fits in every case
    for name, n in (("cap3", 2), ("cap4", 3)):
        pats, nv, consts = ctx.tmpl[name]
        for c in consts:
            assert not lp_ref(adj, pats[:n], c)[1], name
    # the filters after a full table keep every row
    for name in ("cap3-k2k", "cap3-k2c", "cap3-type"):
        assert ctx.ref[name, 0] == (lg.ROWS3, False), name
        assert len(ctx.tmpl[name][0]) == 4
    # a trailing filter that would bring the table far below the cap
    assert ctx.ref["cap3-shrink", 1] == (1, True)
    assert ctx.ref["cap3-shrink", 0] == (0, False)


def test_eight_ops(ctx):
    pats, nv, consts = ctx.tmpl["eight"]
    assert len(pats) == 8 and nv >= 5
    objs = [p[3] for p in pats if p[3] < 0]
    assert len(set(objs)) == nv                    # nv columns at the end
    assert ctx.ref["eight", 0][0] > 0 and ctx.ref["eight", 2][0] > 0
    assert not any(ctx.ref["eight", k][1] for k in range(len(consts)))
    # every prefix still holds rows: no op runs on an empty table
    for n in range(1, 9):
        assert lp_ref(ctx.adj, pats[:n], consts[0])[0] > 0, n


def test_wrong_variants_change_the_count(ctx):
    """What makes a count-only check see a subtly wrong kernel: for every
    constant whose first list fills a wave (63 entries and more) each
    wrong variant's count differs from the right one."""
    for name, variants in lg.WRONG.items():
        pats, nv, consts = ctx.tmpl[name]
        for what, idx, repl in variants:
            bad = lg.wrong_patterns(pats, idx, repl)
            for k, c in enumerate(consts):
                if len(ctx.adj.get((c, P_A, OUT), [])) < 63:
                    continue
                assert lp_ref(ctx.adj, bad, c)[0] != ctx.ref[name, k][0], \
                    (name, what, k)
    for name, idx in lg.STRIDE.items():
        pats, nv, consts = ctx.tmpl[name]
        for k, c in enumerate(consts):
            if len(ctx.adj.get((c, P_A, OUT), [])) < 63:
                continue
            assert lp_ref(ctx.adj, pats, c, restride=idx)[0] != \
                ctx.ref[name, k][0], (name, "stride", k)


def test_exact_overflow_set(ctx):
    got = {key for key, (n, ovf) in ctx.ref.items() if ovf}
    assert got == lg.OVERFLOWS
    assert set(NAMES) == set(ctx.tmpl)


# ---------------------------------------------------------------------
# GPU part
# ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def engines():
    """One engine per graph variant, built once."""
    out = {v: wk.Engine(wk.Store(get_ctx(v).triples), device=0)
           for v in VARIANTS}
    yield out
    out.clear()
    gc.collect()


def _window(eng, tmpl, consts):
    eng.submit_plan_batch(tmpl, consts)
    got = eng.wait_light_batch()
    assert len(got) == len(consts)
    return got.tolist()


def _check_valid_window(eng, cx):
    """A valid window (with an overflow entry in it) is exact."""
    tmpl, consts = cx.template("cap3-type")
    assert _window(eng, tmpl, consts) == cx.want("cap3-type")
    tmpl, consts = cx.template("k2k-lr")
    assert _window(eng, tmpl, consts) == cx.want("k2k-lr")


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_op_sweep(ctx, engines, name):
    """Every template in one window: LP_OVERFLOW exactly where lp_ref
    says overflow, lp_ref's count everywhere else."""
    eng = engines["multi" if ctx.meta["multi"] else "single"]
    tmpl, consts = ctx.template(name)
    got = _window(eng, tmpl, consts)
    assert got == ctx.want(name), (name, got, ctx.want(name))


@pytest.mark.gpu
def test_mixed_window(ctx, engines):
    """Overflowing queries between fitting ones, constants repeated:
    the neighbours are exact and the order is the caller's."""
    eng = engines["multi" if ctx.meta["multi"] else "single"]
    for name in ("cap3", "cap3-shrink", "cap4"):
        tmpl, consts = ctx.template(name)
        fit, ovf = consts
        order = [0, 1, 0, 1, 1, 0, None, 0, 1]
        window = [ctx.meta["absent"] if k is None else consts[k]
                  for k in order]
        want = [0 if k is None else ctx.want(name)[k] for k in order]
        assert want.count(OVF) == 4 and want[0] == want[2] != OVF
        assert _window(eng, tmpl, window) == want, name


@pytest.mark.gpu
def test_window_shapes(ctx, engines):
    """n = 1, 64 and 65, then 3, 300 and 2 back to back on one engine:
    the pinned staging and the device arrays regrow and then run
    under-full."""
    variant = "multi" if ctx.meta["multi"] else "single"
    eng = wk.Engine(wk.Store(ctx.triples), device=0)   # fresh: nothing grown
    for name in ("k2k-lr", "type-inner"):
        tmpl, consts = ctx.template(name)
        want1 = ctx.want(name)
        for n in (1, 64, 65, 3, 300, 2):
            # start at another constant each time
            idx = [(n + i) % len(consts) for i in range(n)]
            got = _window(eng, tmpl, [consts[i] for i in idx])
            assert got == [want1[i] for i in idx], (variant, name, n)


@pytest.mark.gpu
def test_entry_point_state(ctx, engines):
    eng = engines["multi" if ctx.meta["multi"] else "single"]
    tmpl, consts = ctx.template("eight")
    other, oconsts = ctx.template("c2u")
    eng.submit_plan_batch(tmpl, consts)
    with pytest.raises(RuntimeError):            # rc -4: window in flight
        eng.submit_plan_batch(other, oconsts)
    # (a store without a single-type index refuses with ValueError first)
    with pytest.raises((RuntimeError, ValueError)):
        eng.submit_light_batch(oconsts, [P_A] * len(oconsts),
                               [OUT] * len(oconsts), [T_M] * len(oconsts))
    assert eng.wait_light_batch().tolist() == ctx.want("eight")
    # a refused template leaves no window behind
    bad = plan_of(ctx.tmpl["c2u"][0], 1, consts[0], distinct=True)
    with pytest.raises(ValueError):
        eng.submit_plan_batch(bad, consts)
    with pytest.raises(RuntimeError):
        eng.wait_light_batch()
    n = len(eng.run_query(ctx.plan("eight", 0)))
    assert n == ctx.ref["eight", 0][0]
    _check_valid_window(eng, ctx)


def _refusals(cx):
    """name -> template the interpreter must refuse."""
    meta = cx.meta
    a = (int(meta["roots"][3]), P_A, OUT, X)
    two = [a, (X, P_B, OUT, Y)]
    ks = [(-(i + 1), P_U if i % 2 == 0 else P_D, OUT if i % 2 == 0 else IN,
           -(i + 2)) for i in range(8)]
    out = {
        "optional": Plan([a], 2, [X], optional=[(X, P_B, OUT, Y)]),
        "union": Plan([a], 2, [X], unions=[[(X, P_B, OUT, Y)],
                                           [(X, P_C, OUT, Y)]]),
        "offset": plan_of(two, 2, offset=3),
        "distinct": plan_of(two, 2, distinct=True),
        "limit": plan_of(two, 2, limit=5),
        "filter": plan_of(two, 2, filters=[("ne", X, Y)]),
        "predicate variable": plan_of([a, (X, Y, OUT, Z)], 3),
        "constant subject mid-plan":
            plan_of([a, (int(meta["mid"][0]), P_B, OUT, X)], 1),
        "unbound subject": plan_of([a, (Y, P_B, OUT, Z)], 3),
        "index start": plan_of([(T_M, TYPE, IN, X)], 1),
        "9 patterns": plan_of([a] + [(X, P_N, OUT, meta["nconst"])] * 8, 1),
        # eight patterns end at eight columns, so a ninth column takes a
        # ninth pattern and a ninth variable: refused on either count
        "9th column": plan_of([a] + ks, 9),
    }
    # a first-pattern object outside -1 .. -nvars.  Plan() validates at
    # construction only, so shrinking nvars (or replacing the pattern)
    # afterwards reaches the C entry point
    p = plan_of([(a[0], P_A, OUT, Z)], 3)
    p.nvars, p.required_vars = 2, [X]
    out["object past nvars"] = p
    p = plan_of([a], 8)
    p.patterns[0] = (a[0], P_A, OUT, -9)
    out["object past the table"] = p
    return out


@pytest.mark.gpu
def test_refusals(ctx, engines):
    """ValueError (rc -3: fall back to the per-pattern path) for every
    template the interpreter cannot run as asked; nothing a template
    carries is silently dropped.  The engine stays exact."""
    eng = engines["multi" if ctx.meta["multi"] else "single"]
    consts = lg.rc_consts(ctx.meta)
    cases = _refusals(ctx)
    assert cases["object past nvars"].to_c().nvars == 2
    assert cases["object past the table"].to_c().patterns[0].object == -9
    for name, tmpl in cases.items():
        with pytest.raises(ValueError):
            eng.submit_plan_batch(tmpl, consts)
            pytest.fail("accepted: " + name)
        with pytest.raises(RuntimeError):
            eng.wait_light_batch()
        _check_valid_window(eng, ctx)
    # and a plain run_query afterwards
    n = len(eng.run_query(ctx.plan("k2c-3col", 6)))
    assert n == ctx.ref["k2c-3col", 6][0]


@pytest.mark.gpu
def test_partitions(ctx):
    """The op-sweep templates on every rank of W=3 against lp_ref on the
    lists that rank owns: a probe of a key the rank does not own misses,
    and the partition's reference decides overflow."""
    ps = pl.PartSet(ctx.triples, PART_W, oracle=False)
    ps.build_engines(device=0)
    try:
        kept = {name: 0 for name in ctx.tmpl}
        for r, eng in enumerate(ps.engines):
            adj = lg.owned(ctx.adj, r, PART_W)
            for name, (pats, nv, consts) in ctx.tmpl.items():
                ref = [lp_ref(adj, pats, c) for c in consts]
                want = [OVF if o else n for n, o in ref]
                tmpl, cs = ctx.template(name)
                assert _window(eng, tmpl, cs) == want, (r, name)
                kept[name] += sum(n for n, o in ref if not o)
        for name in ctx.tmpl:
            assert (kept[name] > 0) == (fit_rows(ctx, name) > 0), name
    finally:
        ps.close()
        gc.collect()


def _jobs(cx):
    """name -> (start(eng), harvest(eng) -> result, expected)."""
    rc = lg.rc_consts(cx.meta)
    heavy = cx.plan("k2c-3col", 6)

    def batch(name):
        tmpl, consts = cx.template(name)
        return (lambda e: e.submit_plan_batch(tmpl, consts),
                lambda e: e.wait_light_batch().tolist(), cx.want(name))

    return {
        "eight": batch("eight"),
        "cap": batch("cap3-type"),
        "light": (lambda e: e.submit_light_batch(
                      rc, [P_A] * len(rc), [OUT] * len(rc), [T_M] * len(rc)),
                  lambda e: e.wait_light_batch().tolist(),
                  cx.want("type-1col")),
        "submit": (lambda e: e.submit(heavy),
                   lambda e: len(e.fetch_result()),
                   cx.ref["k2c-3col", 6][0]),
    }


@pytest.mark.gpu
def test_overlapping_engines():
    """Three engines on one GpuStore with work in flight at once, the
    batched emulator loop's shape: a plan batch, a light batch and a
    plain submit are all issued before any harvest and harvested in
    reverse order, with the roles rotated over the engines, and with two
    plan batches in flight on two engines.  Every result is the one
    obtained alone, which is lp_ref's."""
    cx = get_ctx("single")
    gstore = wk.GpuStore(wk.Store(cx.triples), device=0)
    engs = [wk.Engine(gstore) for _ in range(3)]
    jobs = _jobs(cx)
    for name, (start, harvest, want) in jobs.items():     # alone
        for e in engs:
            start(e)
            assert harvest(e) == want, ("alone", name)
    rounds = [("eight", "light", "submit"), ("submit", "eight", "light"),
              ("light", "submit", "eight"), ("eight", "cap", "light"),
              ("cap", "submit", "eight")]
    for _ in range(2):
        for roles in rounds:
            for e, name in zip(engs, roles):
                jobs[name][0](e)
            for e, name in reversed(list(zip(engs, roles))):
                assert jobs[name][1](e) == jobs[name][2], (roles, name)
    del engs, gstore
    gc.collect()
