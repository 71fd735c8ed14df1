"""UNION and OPTIONAL groups as part of the asynchronous launch chain:
submit + fetch, graph_build / graph_run, graph_build_suite / graph_launch
and run_query, against the plain expectations of group_async_cases.py
(checked against the oracle by test_group_async_cpu.py), and on LUBM-4
against the oracle itself.  WK_DEV_GROUPS=0 keeps the host-merge path of
run_query and the refusals of the other entry points."""
import numpy as np
import pytest

import wukong_amd as wk
from wukong_amd import Plan, queries as Q
from tests.group_async_cases import Cases, SETS, X, Y, Z, bgp_ref, same
from tests.group_graph import T_START
from tests.oracle_util import sort_rows
from tests.synth_graph import env

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cx():
    return Cases()


@pytest.fixture(scope="module")
def gstore(cx):
    return wk.GpuStore(wk.Store(cx.triples), device=0)


@pytest.fixture(scope="module")
def eng(gstore):
    return wk.Engine(gstore)


def _submit_fetch(e, plan):
    e.submit(plan)
    return e.fetch_result(plan)


# ---- 1. submit + fetch, UNION ----------------------------------------
@pytest.mark.parametrize("shape", ["view-2", "view-1col", "owned-3",
                                   "owned-2", "wide", "empty"])
def test_union_submit(cx, eng, shape):
    """Parents of 1..1025 rows and an empty one, 2 and 3 branches, an
    empty branch, a two-pattern branch that overwrites an owned parent's
    buffer, a parent that is a view, 1 / 2 / 3 / 5 columns."""
    for t in cx.union_parents(shape):
        got = _submit_fetch(eng, cx.union_plan(shape, t))
        assert same(got, cx.union_want(shape, t)), (shape, t, got.shape)
    # run_query takes the same chain
    t = cx.union_parents(shape)[-1]
    assert same(eng.run_query(cx.union_plan(shape, t)), cx.union_want(shape, t))


# ---- 2. submit + fetch, OPTIONAL -------------------------------------
@pytest.mark.parametrize("group", ["k2u", "k2u-type", "k2u-k2u-type",
                                   "k2u-type-k2u", "c2k", "c2k-k2u", "k2k",
                                   "index"])
def test_optional_submit(cx, eng, group):
    """Every group over every start set: the parent is a view of the
    index list, which the group materialises without a host row count."""
    for t in SETS:
        got = _submit_fetch(eng, cx.opt_plan(group, t))
        assert same(got, cx.opt_want(group, t)), (group, t, got.shape)


def test_optional_submit_owned_parent(cx, eng):
    for n in (257, 1025):
        t = T_START[n]
        got = _submit_fetch(eng, cx.opt_owned_plan(t))
        assert same(got, cx.opt_owned_want(t)), n


# ---- 3. UNION, OPTIONAL, FILTER on a group-born variable ---------------
def test_combination_submit(cx, eng):
    for name in cx.combo_filters():
        plan = cx.combo_plan(name)
        assert same(_submit_fetch(eng, plan), cx.combo_want(name)), name
        assert same(eng.run_query(plan), cx.combo_want(name)), name


def test_combination_final_ops(cx, eng, gstore):
    """DISTINCT / OFFSET / LIMIT on the device behind the groups, against
    run_query on the host-merge path."""
    finals = [dict(distinct=True), dict(distinct=True, offset=7, limit=100),
              dict(distinct=True, limit=0), dict(distinct=True, offset=10 ** 6)]
    host = wk.Engine(gstore)
    for name in ("none", "bound", "or"):
        for kw in finals:
            plan = cx.combo_plan(name, **kw)
            plan.required_vars = [Y, Z]
            with env(WK_DEV_GROUPS=0):
                want = host.run_query(plan)
            with env(WK_FINAL_HOST_ROWS=0):
                got = _submit_fetch(eng, plan)
                got2 = eng.run_query(plan)
            assert got.shape == want.shape, (name, kw, got.shape, want.shape)
            assert np.array_equal(got, want), (name, kw)
            assert np.array_equal(got2, want), (name, kw)
    # the count the window cuts from
    full = cx.combo_want("none")
    with env(WK_FINAL_HOST_ROWS=0):
        plan = cx.combo_plan("none", distinct=True)
        assert len(_submit_fetch(eng, plan)) == len(np.unique(full, axis=0))


# ---- 4. graphs -------------------------------------------------------
def _graph_cases(cx):
    return [("union", cx.union_plan("view-2", T_START[513]),
             cx.union_want("view-2", T_START[513])),
            ("union-owned", cx.union_plan("owned-3", T_START[257]),
             cx.union_want("owned-3", T_START[257])),
            ("optional", cx.opt_plan("k2u-type", T_START[513]),
             cx.opt_want("k2u-type", T_START[513])),
            ("combo", cx.combo_plan("bound"), cx.combo_want("bound"))]


def test_graph_build_and_run(cx, gstore):
    """Replays are exact twice over, and a plain-plan graph captured
    BEFORE the group graphs still is after them: no buffer changed
    identity."""
    e = wk.Engine(gstore)
    plain = e.graph_build(cx.PLAIN)
    assert e.graph_run(plain) == len(cx.plain_want())
    gids = [(name, e.graph_build(plan), plan, want)
            for name, plan, want in _graph_cases(cx)]
    for _ in range(2):
        for name, gid, plan, want in gids:
            assert e.graph_run(gid) == len(want), name
            assert same(e.fetch_result(plan), want), name
        assert e.graph_run(plain) == len(cx.plain_want())
        assert same(e.fetch_result(cx.PLAIN), cx.plain_want())


def test_graph_final_ops_behind_groups(cx, gstore):
    e = wk.Engine(gstore)
    plan = cx.combo_plan("none", distinct=True, offset=3, limit=50)
    plan.required_vars = [Y, Z]
    with env(WK_DEV_GROUPS=0):
        want = wk.Engine(gstore).run_query(plan)
    gid = e.graph_build(plan)
    for _ in range(2):
        assert e.graph_run(gid) == len(cx.combo_want("none"))   # blind count
        assert e.final_count() == len(want)
        assert np.array_equal(e.fetch_result(plan), want)


def test_graph_suite(cx, gstore):
    e = wk.Engine(gstore)
    union = cx.union_plan("owned-2", T_START[257])
    opt = cx.opt_plan("k2u-k2u-type", T_START[257])
    for plans, want in (
            ([cx.PLAIN, union, opt, cx.PLAIN], cx.plain_want()),
            ([cx.PLAIN, opt, union], cx.union_want("owned-2", T_START[257])),
            ([union, cx.PLAIN, opt],
             cx.opt_want("k2u-k2u-type", T_START[257]))):
        gid = e.graph_build_suite(plans)
        for _ in range(2):
            e.graph_launch(gid)
            e.sync()
            assert same(e.fetch_result(plans[-1]), want)


def test_graph_hints_stay_with_the_main_patterns(cx, gstore):
    """The warm pass sees main pattern 1 (`?x P_TAG ?z`, one edge per
    row) drop nothing and notes a no-drop hint for step 1.  Step 1 of the
    first UNION branch is a type filter that does drop rows, behind an
    expansion (its step 0) that drops rows too; step 0 itself can have no
    hint, the first pattern of a plan never has one.  A replay that took
    the main pattern's hint for the branch would verify instead of filter
    and come back as an overflow."""
    e = wk.Engine(gstore)
    for shape in ("owned-3", "owned-2"):
        for t in (T_START[257], T_START[1025]):
            plan, want = cx.union_plan(shape, t), cx.union_want(shape, t)
            main = cx.union_main(shape, t)
            first = cx.union_shapes()[shape][1][0]
            assert len(bgp_ref(cx.adj, main)[0]) == len(cx.members(t))
            expanded = len(bgp_ref(cx.adj, main + first[:1])[0])
            kept = len(cx.branch_tables(shape, t)[0])
            assert 0 < kept < expanded, (shape, t)    # the filter drops rows
            gid = e.graph_build(plan)
            for _ in range(2):
                assert e.graph_run(gid) == len(want), (shape, t)
                assert same(e.fetch_result(plan), want), (shape, t)


# ---- 5. overflow -----------------------------------------------------
def test_union_overflow(cx, gstore):
    """Each branch fits the capacity, their sum does not: the append
    clamps and flags, the fetch reports it and grows, the second submit is
    exact; run_query does all of that in one call."""
    t = T_START[1025]
    a, b = [len(p) for p in cx.branch_tables("view-2", t)]
    cap = max(a, b) + 8
    assert a <= cap and b <= cap and a + b > cap and len(cx.members(t)) <= cap
    plan, want = cx.union_plan("view-2", t), cx.union_want("view-2", t)
    with env(WK_MIN_CAP=cap):
        e = wk.Engine(gstore)
        e.submit(plan)
        with pytest.raises(RuntimeError, match="rc=-5"):
            e.fetch_result(plan)
        assert same(_submit_fetch(e, plan), want)
        assert same(wk.Engine(gstore).run_query(plan), want)
        # three branches, the overflow in the middle of the merge
        plan3 = cx.union_plan("owned-3", t)
        assert same(wk.Engine(gstore).run_query(plan3),
                    cx.union_want("owned-3", t))


def test_optional_overflow(cx, gstore):
    t = T_START[1025]
    want = cx.opt_want("k2u", t)
    cap = 2000
    assert len(cx.members(t)) <= cap < len(want)
    plan = cx.opt_plan("k2u", t)
    with env(WK_MIN_CAP=cap):
        e = wk.Engine(gstore)
        e.submit(plan)
        with pytest.raises(RuntimeError, match="rc=-5"):
            e.fetch_result(plan)
        assert same(_submit_fetch(e, plan), want)
        assert same(wk.Engine(gstore).run_query(plan), want)
        plan2 = cx.opt_plan("k2u-k2u-type", t)
        assert same(wk.Engine(gstore).run_query(plan2),
                    cx.opt_want("k2u-k2u-type", t))


# ---- 6. knob ---------------------------------------------------------
def test_knob_off(cx, gstore):
    e = wk.Engine(gstore)
    cases = [(cx.union_plan("owned-3", T_START[513]),
              cx.union_want("owned-3", T_START[513])),
             (cx.opt_plan("k2u-type", T_START[513]),
              cx.opt_want("k2u-type", T_START[513])),
             (cx.combo_plan("or"), cx.combo_want("or"))]
    for plan, want in cases:
        on = e.run_query(plan)
        with env(WK_DEV_GROUPS=0):
            with pytest.raises(RuntimeError, match="rc=-3"):
                e.submit(plan)
            with pytest.raises(RuntimeError, match="rc=-3"):
                e.graph_build(plan)
            with pytest.raises(RuntimeError, match="rc=-3"):
                e.graph_build_suite([cx.PLAIN, plan])
            off = e.run_query(plan)
        assert same(on, want) and same(off, want)
        assert np.array_equal(sort_rows(on), sort_rows(off))
    # plain plans are untouched by the knob
    with env(WK_DEV_GROUPS=0):
        assert same(_submit_fetch(e, cx.PLAIN), cx.plain_want())


# ---- 7. LUBM-4 against the oracle --------------------------------------
def _lubm_plans():
    union = Plan([(Q.GRADSTUDENT, Q.TYPE_ID, wk.DIR_IN, X)], 2, [X, Y],
                 unions=[[(X, Q.MEMBEROF, wk.DIR_OUT, Y)],
                         [(X, Q.UGDEGREE, wk.DIR_OUT, Y)]])
    opt = Plan([(Q.UGSTUDENT, Q.TYPE_ID, wk.DIR_IN, X)], 2, [X, Y],
               optional=[(X, Q.ADVISOR, wk.DIR_OUT, Y)])
    opt2 = Plan([(Q.UGSTUDENT, Q.TYPE_ID, wk.DIR_IN, X)], 2, [X, Y],
                optional=[(X, Q.ADVISOR, wk.DIR_OUT, Y),
                          (Y, Q.TYPE_ID, wk.DIR_OUT, Q.FULLPROF)])
    both = Plan([(Q.GRADSTUDENT, Q.TYPE_ID, wk.DIR_IN, X)], 3, [X, Y, Z],
                unions=[[(X, Q.MEMBEROF, wk.DIR_OUT, Y)],
                        [(X, Q.UGDEGREE, wk.DIR_OUT, Y)]],
                optional=[(X, Q.ADVISOR, wk.DIR_OUT, Z)])
    return dict(union=union, opt=opt, opt2=opt2, both=both)


def test_lubm4_submit_and_graph(store4, oracle4):
    e = wk.Engine(store4, device=0)
    for name, plan in _lubm_plans().items():
        want = sort_rows(oracle4.run_query(plan))
        assert len(want) > 0, name
        assert same(_submit_fetch(e, plan), want), name
        gid = e.graph_build(plan)
        assert e.graph_run(gid) == len(want), name
        assert same(e.fetch_result(plan), want), name
