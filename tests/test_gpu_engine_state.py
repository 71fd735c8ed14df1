"""Host state of the engine across refused graph builds, the two capture
routes, the step path's overflow re-run and UNION.

The engine keeps "where the table is" (current buffer, zero-copy view,
column count, row bound, variable -> column map) and a few mode flags
(hint pass, capture, OPTIONAL group, whole-plan run) as plain fields that
several paths save, set and put back.  These cases pin what a slip there
would break, on the 2049-subject graph of test_gpu_chain_width (with the
two extra predicates of test_gpu_chain_sched) and against the oracle;
rows are compared as sorted multisets.

 - a graph build that is refused, before anything ran, behind another
   plan's warm pass or inside the capture, leaves no flag behind: the same
   engine then runs chain-fused plans with the rows and the per-category launch
   counts of a fresh engine, and builds and replays them;
 - a one-plan suite graph is the single build's chain: graph_run and
   graph_launch + sync + row_count give the same count, with and without a
   truncated empty tail (expect_empty is passed on both routes);
 - the step API's overflow re-run sees its zero-copy input again;
 - UNION branches restart from a parent that is a zero-copy view.
"""
import pytest

import wukong_amd as wk
from wukong_amd import Plan
from tests import test_gpu_chain_sched as S
from tests import test_gpu_chain_width as W
from tests.oracle_util import OracleCtx, sort_rows
from tests.synth_graph import IN, OUT, TYPE, env

A_, B_ = -1, -2


class Ctx:
    def __init__(self):
        self.triples, self.meta = S.sched_graph()
        self.ora = OracleCtx(self.triples)
        self._want = {}

    def plan(self, name, n):
        for mk in (W.plans, S.row_plans, S.exp_plans):
            d = mk(n, self.meta)
            if name in d:
                return d[name]
        raise KeyError(name)

    def want(self, key, plan):
        if key not in self._want:
            r = sort_rows(self.ora.run_query(plan))
            r.setflags(write=False)
            self._want[key] = r
        return self._want[key]


@pytest.fixture(scope="module")
def ctx():
    return Ctx()


@pytest.fixture(scope="module")
def gstore(ctx):
    return wk.GpuStore(wk.Store(ctx.triples), device=0)


def _launches(eng, plan):
    """Rows of run_query and the launches it made, per category."""
    before = {k: v["launches"] for k, v in eng.kernel_stats().items()}
    rows = sort_rows(eng.run_query(plan))
    after = {k: v["launches"] for k, v in eng.kernel_stats().items()}
    return rows, {k: after[k] - before[k] for k in after}


@pytest.mark.gpu
def test_no_mode_flag_survives_a_refused_build(ctx, gstore):
    with env(WK_KERNEL_TIMING=1):
        eng = wk.Engine(gstore)
        fresh = wk.Engine(gstore)
    fused = {k: ctx.plan(k, 1025) for k in ("rp3", "x-q7")}
    rp3 = fused["rp3"]
    distinct = Plan(rp3.patterns, rp3.nvars, rp3.required_vars, distinct=True)
    with env(WK_DEV_FINAL=0):
        with pytest.raises(RuntimeError, match="rc=-3"):
            eng.graph_build(distinct)
        # refused after the warm and hint pass of the plan in front of it
        with pytest.raises(RuntimeError, match="rc=-3"):
            eng.graph_build_suite([rp3, distinct])
        with pytest.raises(RuntimeError, match="rc=-3"):
            eng.graph_build_suite([distinct])
    # refused INSIDE the capture: nine required vars are more than the
    # device final pass takes, which is found out once the chain has been
    # recorded; the capture is abandoned, as a single build and as the
    # second plan of a suite
    nine = Plan(rp3.patterns, rp3.nvars, rp3.required_vars * 3, distinct=True)
    assert len(nine.required_vars) == 9
    for build in (lambda: eng.graph_build(nine),
                  lambda: eng.graph_build_suite([rp3, nine])):
        with pytest.raises(RuntimeError, match="rc=-3"):
            build()
    for key, plan in fused.items():
        want = ctx.want(key, plan)
        assert len(want) > 0, key
        got, n_got = _launches(eng, plan)
        ref, n_ref = _launches(fresh, plan)
        print(key, "launches", n_got, "fresh", n_ref)
        assert W._same(got, want), (key, got.shape, want.shape)
        assert W._same(ref, want), (key, ref.shape, want.shape)
        assert n_got == n_ref, (key, n_got, n_ref)
        with env(WK_CHAIN=0):                  # the plans ARE chain-fused
            _, n_off = _launches(fresh, plan)
        assert sum(n_ref.values()) < sum(n_off.values()), (key, n_ref, n_off)
        gid = eng.graph_build(plan)
        assert eng.graph_run(gid) == len(want), key
        assert W._same(sort_rows(eng.fetch_result(plan)), want), key


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rp3", "x-q7", "none", "x-none"])
def test_suite_of_one_is_the_single_chain(ctx, gstore, name):
    """`none` and `x-none` are empty from their second / third pattern on:
    both builds truncate the tail and publish with expect_empty."""
    eng = wk.Engine(gstore)
    plan = ctx.plan(name, 1025)
    want = ctx.want(name, plan)
    assert (len(want) == 0) == name.endswith("none")
    gid = eng.graph_build(plan)
    sid = eng.graph_build_suite([plan])
    for _ in range(2):
        single = eng.graph_run(gid)
        eng.graph_launch(sid)
        eng.sync()
        suite = eng.row_count()
        print(name, "single", single, "suite", suite, "oracle", len(want))
        assert single == suite == len(want), name
        assert W._same(sort_rows(eng.fetch_result(plan)), want), name


@pytest.mark.gpu
@pytest.mark.parametrize("n,cap", [(64, 64), (1025, 2048)])
def test_step_rerun_sees_its_view_again(ctx, gstore, n, cap):
    """The index start is a zero-copy view of n rows (n <= cap); the
    expansion behind it overflows the capacity, and the re-run of that step
    must read the view, not the owned buffer."""
    plan = W._plan([(W.r_type(n), TYPE, IN, A_), (A_, W.P_E, OUT, B_)], 2)
    want = ctx.want("step-n%d" % n, plan)
    assert len(want) > cap >= n
    with env(WK_MIN_CAP=cap):
        eng = wk.Engine(gstore)
        eng.begin_query(plan)
        assert eng.execute_one_pattern() == n
        assert eng.execute_one_pattern() == len(want)
        got = sort_rows(eng.fetch_result(plan))
    assert W._same(got, want), (n, got.shape, want.shape)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [64, 1025])
def test_union_after_a_view(ctx, gstore, n):
    """The parent of the branches is the bare index start: the second
    branch restarts from the snapshot, materialised in the owned buffer."""
    plan = Plan([(W.r_type(n), TYPE, IN, A_)], 2, [A_, B_],
                unions=[[(A_, W.P_G, OUT, B_)], [(A_, W.P_E, OUT, B_)]])
    want = ctx.want("union-n%d" % n, plan)
    assert len(want) > 2 * n
    eng = wk.Engine(gstore)
    for _ in range(2):
        got = sort_rows(eng.run_query(plan))
        assert W._same(got, want), (n, got.shape, want.shape)
