"""Captured-plan replays after the bookkeeping launches were removed.

Three things changed in how a captured plan keeps its device state, and
each has a failure mode that only shows in a replay:

* the optimistic kernels (k_expand_fn_map, the verify-only k_filter_tpr,
  the verify-fused k_expand_in / k_expand_big) count guard misses into
  one sticky word that only the publish turns into S_ERR — a miss in an
  EARLY step must survive every later step, and nothing may depend on
  the S_TOTAL / S_OVF resets the per-step commits used to do;
* the begin zeroing rides on the query's first state write — flags of a
  previous query must not leak, and a continuation that starts with
  load_rbuf must still begin clean;
* patterns that the build's warm pass saw run on an empty table are
  host bookkeeping only — the post-replay table layout must be the full
  run's, and the guard must discard the replay when the table is not
  empty after all (WK_FORCE_EMPTY_HINT, test-only).

Whole plans of test_gpu_operator_edges.py run on its synthetic graph;
the multi-step plans run on `chain_graph()` below.  The references are
the oracle (and, on the CPU side, the brute-force matcher it is checked
against).  An OverflowError from graph_run / sync is the engine's error
return for a discarded replay, not a GPU fault.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import wukong_amd as wk
from wukong_amd import Plan
from tests import synth_graph as sg
from tests import test_gpu_operator_edges as T
from tests.oracle_util import OracleCtx, sort_rows
from tests.synth_graph import B, IN, OUT, TYPE

# ---------------------------------------------------------------------
# chain graph: index start -> fn expansion (+ fused type filter) ->
# const filter -> non-functional expansion -> type filter, every step
# after the start keeping every row
# ---------------------------------------------------------------------
P_F, P_G, P_M = 2, 3, 4          # functional / to one constant / 1..40 edges
T_A, T_B, T_NONE = 10, 11, 12    # T_NONE has no member
ROWS = (1023, 1024, 1025)        # around the 1024-row filter tile
WHERE = ("first", "last", "none")
NB = 64
BIG_DEG = 40                     # > 32: the wave-per-row expansion pass


def start_type(where, n):
    return 20 + 3 * WHERE.index(where) + ROWS.index(n)


def chain_graph():
    """(triples, meta).  One start set per (where, n): n subjects of
    their own type.  `where` places the one entity typed T_A + T_B —
    a guard miss for the optimistic kernels when the store has no type
    bitmaps — in the fn expansion ("first"), in the non-functional
    expansion ("last": a 1-edge row for odd n, the 40-edge row for
    n == 1024) or nowhere ("none")."""
    nxt = [B]

    def take(k):
        a = np.arange(nxt[0], nxt[0] + k, dtype=np.uint32)
        nxt[0] += k
        return a

    trip = []

    def add(s, p, o):
        s, o = np.broadcast_arrays(np.asarray(s, np.uint32),
                                   np.asarray(o, np.uint32))
        trip.append(np.stack([s.ravel(), np.full(s.size, p, np.uint32),
                              o.ravel()], axis=1))

    nb = take(NB)
    multi, c0 = int(take(1)[0]), int(take(1)[0])
    add(nb, TYPE, T_B)
    add([multi, multi], TYPE, [T_A, T_B])
    subjects = {}
    for where in WHERE:
        for n in ROWS:
            s = take(n)
            i = np.arange(n)
            fo = nb[i % NB].copy()
            if where == "first":
                fo[7] = multi
            add(s, P_F, fo)
            add(s, P_G, c0)
            mo = nb[(i + 1) % NB].copy()
            if where == "last" and n != 1024:
                mo[9] = multi
            add(s, P_M, mo)
            add(s[::5], P_M, nb[(i[::5] + 2) % NB])
            big = nb[:BIG_DEG].copy()
            if where == "last" and n == 1024:
                big[BIG_DEG - 1] = multi
            add(s[3], P_M, big)
            add(s, TYPE, start_type(where, n))
            subjects[(where, n)] = s
    triples = np.unique(np.concatenate(trip).astype(np.uint32), axis=0)
    return triples, dict(nb=nb, multi=multi, c0=c0, subjects=subjects)


def chain_plan(where, n, c0):
    """Three no-drop steps in a row after the start: fn expansion with
    its fused type filter, const filter, expansion + type filter."""
    return Plan([(start_type(where, n), TYPE, IN, -1),
                 (-1, P_F, OUT, -2), (-2, TYPE, OUT, T_B),
                 (-1, P_G, OUT, c0),
                 (-1, P_M, OUT, -3), (-3, TYPE, OUT, T_B)],
                nvars=3, required_vars=[-1, -2, -3])


def empty_plans(c0):
    """name -> (plan, index of the last pattern with rows or None)."""
    t = start_type("none", 1023)
    tail = [(-1, P_F, OUT, -2), (-1, P_M, OUT, -3), (-3, TYPE, OUT, T_B)]
    return {
        # no member of the start type at all
        "after-0": Plan([(T_NONE, TYPE, IN, -1)] + tail, nvars=3,
                        required_vars=[-1, -2, -3]),
        # no start subject is a T_A
        "middle": Plan([(t, TYPE, IN, -1), (-1, P_G, OUT, c0),
                        (-1, TYPE, OUT, T_A)] + tail, nvars=3,
                       required_vars=[-1, -2, -3]),
        # empty only once the last pattern ran: nothing to truncate
        "last": Plan([(t, TYPE, IN, -1), (-1, P_M, OUT, -2),
                      (-2, TYPE, OUT, T_A)], nvars=2,
                     required_vars=[-1, -2]),
        "never": chain_plan("none", 1023, c0),
    }


STORES = ("default", "notbm", "hash")


class ChainCtx:
    def __init__(self):
        self.triples, self.meta = chain_graph()
        self.ora = OracleCtx(self.triples)
        self._want = {}

    def want(self, key, plan):
        if key not in self._want:
            w = sort_rows(self.ora.run_query(plan))
            w.setflags(write=False)
            self._want[key] = w
        return self._want[key]


@pytest.fixture(scope="module")
def cctx():
    return ChainCtx()


@pytest.fixture(scope="module")
def ectx():
    return T.Ctx()


def _engines(triples):
    out = {}
    for name in STORES:
        with sg.env(**T.STORE_ENVS[name]):
            out[name] = wk.Engine(wk.Store(triples), device=0)
    return out


@pytest.fixture(scope="module")
def chain_engines(cctx):
    return _engines(cctx.triples)


@pytest.fixture(scope="module")
def edge_engines(ectx):
    return _engines(ectx.triples)


# ---------------------------------------------------------------------
# CPU part: the chain graph has the shape the GPU tests rely on
# ---------------------------------------------------------------------
def test_chain_graph_shape(cctx):
    meta = cctx.meta
    store = wk.Store(cctx.triples)
    assert store.check() == 0
    k, e = store.seg_stats(P_F, OUT)
    assert k == e > 0                      # functional
    k, e = store.seg_stats(P_M, OUT)
    assert 0 < k < e                       # not functional
    assert list(store.get_triples(meta["multi"], TYPE, OUT)) == [T_A, T_B]
    assert len(store.get_index(T_NONE, IN)) == 0
    for (where, n), s in meta["subjects"].items():
        assert len(store.get_index(start_type(where, n), IN)) == n
        assert len(store.get_triples(int(s[3]), P_M, OUT)) == BIG_DEG > 32
        plan = chain_plan(where, n, meta["c0"])
        want = cctx.want((where, n), plan)
        # no step drops a row: the result is every (s, f(s), m) triple
        n_m = sum(len(store.get_triples(int(v), P_M, OUT)) for v in s)
        assert len(want) == n_m > n
        assert np.array_equal(want, sort_rows(cctx.ora.brute_query(plan)))
        has_multi = {c: bool((want[:, c] == meta["multi"]).any())
                     for c in (1, 2)}
        assert has_multi == {1: where == "first", 2: where == "last"}


def test_empty_plans_shape(cctx):
    plans = empty_plans(cctx.meta["c0"])
    for name, plan in plans.items():
        want = cctx.want(("empty", name), plan)
        assert (len(want) == 0) == (name != "never"), name
        assert np.array_equal(want, sort_rows(cctx.ora.brute_query(plan)))
    # "last" has rows until its final pattern
    head = Plan(plans["last"].patterns[:2], nvars=2, required_vars=[-1, -2])
    assert len(cctx.ora.run_query(head)) > 0
    head = Plan(plans["middle"].patterns[:2], nvars=3, required_vars=[-1])
    assert len(cctx.ora.run_query(head)) == 1023


# ---------------------------------------------------------------------
# GPU part
# ---------------------------------------------------------------------
def _replay(eng, gid):
    """Row count of one replay, None when the engine discarded it."""
    try:
        return eng.graph_run(gid)
    except OverflowError:
        return None


def _check_run_query(eng, plan, want, tag):
    got = eng.run_query(plan)
    assert got.shape == want.shape, (tag, "run_query", got.shape, want.shape)
    assert np.array_equal(sort_rows(got), want), (tag, "run_query")


def _check_replays(eng, plan, want, tag, may_miss):
    """graph_build, two replays, the table a replay leaves, then the
    plain path on the same engine."""
    gid = eng.graph_build(plan)
    for i in range(2):
        n = _replay(eng, gid)
        print(tag, "replay", i, "rows", n, "want", len(want))
        if n is None:
            assert may_miss, (tag, "replay discarded")
            continue
        assert n == len(want), (tag, n, len(want))
        raw = eng.fetch_raw()
        assert raw.shape == want.shape, (tag, "raw", raw.shape, want.shape)
        assert np.array_equal(sort_rows(raw), want), (tag, "raw")
    _check_run_query(eng, plan, want, tag)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(T.PLANS) + list(T.MISS_PLANS))
@pytest.mark.parametrize("config", ["default", "default-nofn", "notbm", "hash"])
def test_replay_parity_and_state(ectx, edge_engines, config, name):
    """Every whole plan of the operator-edge tests, under the store
    configurations that select the three optimistic kernels differently:
    two replays give the oracle count, fetch_raw after a replay gives
    the oracle rows (the plans' required vars are all columns, in
    binding order), and run_query afterwards still matches.  The
    MISS_PLANS hold a multi-typed entity: where the kernels have no type
    bitmap the replay may be discarded instead, never wrong."""
    store, kv = T.CONFIGS[config]
    eng = edge_engines[store]
    plan = {**T.PLANS, **T.MISS_PLANS}[name]
    want = ectx.want(name, plan)
    may_miss = name in T.MISS_PLANS and store != "default"
    with sg.env(**kv):
        _check_replays(eng, plan, want, (config, name), may_miss)


@pytest.mark.gpu
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("store", STORES)
def test_miss_survives_later_steps(cctx, chain_engines, store, where, n):
    """fn expansion, verify-only filter and verify-fused expansion in
    one captured plan, 1023 / 1024 / 1025 rows at the filter.  The
    multi-typed entity sits in the first optimistic step or in the last:
    the replay is exact (bitmaps decide it) or discarded, and the safe
    path gives the oracle rows."""
    eng = chain_engines[store]
    plan = chain_plan(where, n, cctx.meta["c0"])
    want = cctx.want((where, n), plan)
    _check_replays(eng, plan, want, (store, where, n),
                   may_miss=store != "default")


@pytest.mark.gpu
@pytest.mark.parametrize("store", STORES)
def test_no_miss_is_not_discarded(cctx, chain_engines, store):
    """The same three optimistic steps with nothing to miss: no leftover
    cursor or queue length of one step may read as a miss of the next
    (the 40-edge row leaves the big-row queue non-empty)."""
    eng = chain_engines[store]
    for n in ROWS:
        plan = chain_plan("none", n, cctx.meta["c0"])
        _check_replays(eng, plan, cctx.want(("none", n), plan), (store, n),
                       may_miss=False)


@pytest.mark.gpu
@pytest.mark.parametrize("store", STORES)
def test_empty_tail(cctx, chain_engines, store):
    eng = chain_engines[store]
    plans = empty_plans(cctx.meta["c0"])
    for name, plan in plans.items():
        want = cctx.want(("empty", name), plan)
        eng.submit(plan)
        full = eng.fetch_raw()          # the full run's layout
        gid = eng.graph_build(plan)
        for _ in range(2):
            assert eng.graph_run(gid) == len(want), (store, name)
            raw = eng.fetch_raw()
            assert raw.shape == full.shape, (store, name, raw.shape, full.shape)
            if name != "never":
                assert raw.shape == (0, 3 if name != "last" else 2)
        _check_run_query(eng, plan, want, (store, name))
    # one capture: a non-empty plan before and after each empty one
    never = plans["never"]
    other = chain_plan("none", 1025, cctx.meta["c0"])
    w_other = cctx.want(("none", 1025), other)
    for name in ("after-0", "middle", "last"):
        gid = eng.graph_build_suite([never, plans[name], other])
        for _ in range(2):
            eng.graph_launch(gid)
            eng.sync()
        raw = eng.fetch_raw()
        assert raw.shape == w_other.shape, (store, name, raw.shape)
        assert np.array_equal(sort_rows(raw), w_other), (store, name)
        _check_run_query(eng, plans[name], cctx.want(("empty", name),
                                                     plans[name]),
                         (store, name, "after suite"))


@pytest.mark.gpu
def test_load_rbuf_continuation(cctx, chain_engines):
    """begin_query + load_rbuf at step > 0 (the distributed driver's
    continuation): the begin zeroing is done by the load's state write."""
    eng = chain_engines["default"]
    meta = cctx.meta
    plan = chain_plan("none", 1025, meta["c0"])
    want = cctx.want(("none", 1025), plan)
    table = meta["subjects"][("none", 1025)].reshape(-1, 1)
    for _ in range(2):
        eng.begin_query(plan)
        eng.load_rbuf(table, [0, -1, -1], 1)
        while eng.pattern_step < len(plan.patterns):
            eng.execute_one_pattern()
        got = eng.fetch_raw()
        assert got.shape == want.shape, (got.shape, want.shape)
        assert np.array_equal(sort_rows(got), want)


_CHILD_HEAD = """
import os, sys
sys.path.insert(0, %r)
import numpy as np
import wukong_amd as wk
from tests import synth_graph as sg
from tests import test_graph_replay_bookkeeping as R
from tests import test_gpu_operator_edges as T
from tests.oracle_util import OracleCtx, sort_rows
"""

_GUARD_CHILD = _CHILD_HEAD + """
triples, meta = R.chain_graph()
ora = OracleCtx(triples)
eng = wk.Engine(wk.Store(triples), device=0)
plan = R.chain_plan('none', 1023, meta['c0'])
other = R.chain_plan('none', 1025, meta['c0'])
want = sort_rows(ora.run_query(plan))
assert len(want) > 0
os.environ['WK_FORCE_EMPTY_HINT'] = '0'     # pattern 0 leaves 1023 rows
gid = eng.graph_build(plan)
sid = eng.graph_build_suite([other, plan, other])
del os.environ['WK_FORCE_EMPTY_HINT']
for _ in range(2):
    try:
        n = eng.graph_run(gid)
        raise SystemExit('replay not discarded: %%r' %% (n,))
    except OverflowError:
        pass
    got = eng.run_query(plan)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(sort_rows(got), want)
eng.graph_launch(sid)
try:
    eng.sync()
    raise SystemExit('suite replay not discarded')
except OverflowError:
    pass
got = eng.run_query(plan)
assert got.shape == want.shape and np.array_equal(sort_rows(got), want)
# a build without the knob replays fine on the same engine
gid = eng.graph_build(plan)
assert eng.graph_run(gid) == len(want)
print('EMPTY_GUARD_OK')
"""

_BEGIN_CHILD = _CHILD_HEAD + """
os.environ['WK_MIN_CAP'] = '1000'
triples, meta = sg.edge_graph()
ora = OracleCtx(triples)
with sg.env(**T.STORE_ENVS['hash']):
    gstore = wk.GpuStore(wk.Store(triples), device=0)
plan = T.PLANS['hub-ladder']
small = T.PLANS['fn-nodrop']
want = sort_rows(ora.run_query(plan))
w_small = sort_rows(ora.run_query(small))
eng = wk.Engine(gstore)
eng.submit(plan)
assert eng.fetch_count() == -1      # overflowed at 1000 rows: S_ERR, grown
# the next query on the same engine starts clean
eng.submit(small)
got = eng.fetch_result()
assert got.shape == w_small.shape, (got.shape, w_small.shape)
assert np.array_equal(sort_rows(got), w_small)
eng.submit(plan)
n = eng.fetch_count()
while n < 0:
    eng.submit(plan)
    n = eng.fetch_count()
assert n == len(want), (n, len(want))
eng.submit(plan)
got = eng.fetch_result()
assert got.shape == want.shape and np.array_equal(sort_rows(got), want)
print('BEGIN_STATE_OK')
"""


def _child(src, token):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", src % (root,)],
                       capture_output=True, text=True, timeout=300)
    assert token in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_empty_guard_discards_replay():
    """WK_FORCE_EMPTY_HINT=0 on a plan whose pattern 0 leaves 1023 rows:
    graph_run and the suite's sync raise OverflowError, run_query after
    either returns the oracle rows."""
    _child(_GUARD_CHILD, "EMPTY_GUARD_OK")


@pytest.mark.gpu
def test_begin_after_flagged_query():
    """WK_MIN_CAP=1000: a submit that overflowed and flagged S_ERR, then
    submit + fetch_result of another plan on the same engine."""
    _child(_BEGIN_CHILD, "BEGIN_STATE_OK")
