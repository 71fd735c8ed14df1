"""Per-row op chains: a run of 1:1 patterns fused into
the CSR expansion they follow, as its per-edge predicate (LUBM Q7's
shape).

The graph below is built for this file: functional (forward and
reversed-only) predicates with absent keys, exact multi-typed and
untyped objects, a degree ladder around the 32- and 64-edge row classes
with a hub, and one start set per input row count.  Every comparison is
exact: sorted row sets against the oracle and against the same engine
with WK_CHAIN=0.

CPU part (unmarked): oracle == brute for every plan of the file, and
the graph has the properties the GPU cases rely on.
"""
import numpy as np
import pytest

import wukong_amd as wk
from wukong_amd import Plan
from tests.oracle_util import OracleCtx, OracleExecutor, sort_rows
from tests.synth_graph import B, IN, OUT, TYPE, env

ROWS = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049]
WIDE_ROWS = [0, 1, 65, 257]        # start rows of the hub-fed 2-column case
N_SMALL = 2049

# predicates
P_M, P_U, P_SUB, P_ONE, P_W, P_NM2, P_TK, P_TCH, P_NM, P_HB = range(2, 12)
# types
T_D, T_U, T_X, T_ANY, T_C, T_L, T_ALL = range(20, 27)
T_S0 = 40                          # T_S0 + i: first ROWS[i] students
T_P0 = 60                          # T_P0 + i: first ROWS[i] professors
ND, NU, NCRS, HUB = 64, 16, 997, 7
LAD = [0, 1, 2, 3, 32, 33, 64, 65, 5, 2, 1, 1, 3, 130]
HUB_DEG = 700
HUB_PASS = [10, 63, 64, 65, 127, 128, 300, 699]   # passing edge positions
INV3 = 665                         # 3 * 665 == 1 (mod 997)
D0 = B + N_SMALL                   # vid of department 0 in the small graph

STORE_ENVS = {
    "default": {},
    "hash": dict(WK_FN=0, WK_CSR=0, WK_TBM=0),
    "notbm": dict(WK_TBM=0),
}


def s_type(n):
    return T_S0 + ROWS.index(n)


def p_type(n):
    return T_P0 + ROWS.index(n)


def chain_graph(nstud):
    """(triples, meta) with `nstud` students and N_SMALL professors."""
    nxt = [B]

    def take(n):
        a = np.arange(nxt[0], nxt[0] + n, dtype=np.uint32)
        nxt[0] += n
        return a

    trip = []

    def add(s, p, o):
        s, o = np.broadcast_arrays(np.asarray(s, np.uint32),
                                   np.asarray(o, np.uint32))
        trip.append(np.stack([s.ravel(), np.full(s.size, p, np.uint32),
                              o.ravel()], axis=1))

    S, D, U = take(nstud), take(ND), take(NU)
    Pr, C, L = take(N_SMALL), take(NCRS), take(NCRS)
    i = np.arange(nstud)
    # students: memberOf (always), ugDegreeFrom (key absent when i % 3 == 0)
    add(S, P_M, D[i % ND])
    has_u = i % 3 != 0
    add(S[has_u], P_U, U[(i[has_u] * 7) % NU])
    add(S[:1], P_ONE, D[:1])                     # a one-key functional map
    w = i % 64 == 0
    add(S[w], P_W, D[0])                         # one key per 64 students
    add(S[i % 2 == 0], P_NM2, L[i[i % 2 == 0] % NCRS])
    # departments: subOrgOf (functional OUT, not IN); D[5] untyped, D[6]
    # multi-typed; every department is T_ANY
    add(D, P_SUB, U[np.arange(ND) % NU])
    j = np.arange(ND)
    add(D[j != 5], TYPE, T_D)
    add(D[6], TYPE, T_X)
    add(D, TYPE, T_ANY)
    k = np.arange(NU)
    add(U[k != 3], TYPE, T_U)
    add(U[3], TYPE, T_X)
    add(L, TYPE, T_L)
    # courses: T_C unless m % 4 == 1 (T_X); m % 16 == 2 has both
    m = np.arange(NCRS)
    add(C[m % 4 != 1], TYPE, T_C)
    add(C[(m % 4 == 1) | (m % 16 == 2)], TYPE, T_X)
    add(C[m % 5 != 0], P_NM, L[m[m % 5 != 0]])   # name: key absent if m%5==0
    # takesCourse ladder + hub; teacherOf: each course has ONE teacher, the
    # professor whose first course it is, except the hub's passing edges
    teacher = (m * INV3) % NCRS
    for q in range(N_SMALL):
        deg = HUB_DEG if q == HUB else LAD[q % len(LAD)]
        if deg:
            add(Pr[q], P_TK, C[(3 * q + 5 * np.arange(deg)) % NCRS])
    for pos in HUB_PASS:
        teacher[(3 * HUB + 5 * pos) % NCRS] = HUB
    add(Pr[teacher], P_TCH, C)
    # hub-class predicate (avg degree 40 > 32: never the typeof-fused path)
    for q in range(N_SMALL):
        add(Pr[q], P_HB, S[(40 * q + np.arange(40)) % min(nstud, N_SMALL)])
    for n in ROWS:
        if n:
            add(S[:n], TYPE, s_type(n))
            add(Pr[:n], TYPE, p_type(n))
    add(S, TYPE, T_ALL)
    meta = dict(S=S, D=D, U=U, Pr=Pr, C=C, L=L)
    return np.concatenate(trip).astype(np.uint32), meta


X, Y, Z, W = -1, -2, -3, -4


def _same(got, want):
    """Exact equality of two sorted row sets (an empty result has no
    column count worth comparing)."""
    if len(got) == 0 or len(want) == 0:
        return len(got) == len(want)
    return got.shape == want.shape and np.array_equal(got, want)


def _plan(pats, nvars):
    return Plan(pats, nvars=nvars,
                required_vars=[-(v + 1) for v in range(nvars)])


def tail_plans(t):
    """CSR expansion with a fused trailing chain (professor start)."""
    a, b, c, d, e = -1, -2, -3, -4, -5
    s0 = (t, TYPE, IN, a)
    sS = (t - T_P0 + T_S0, TYPE, IN, a)      # the student set of the same size
    mem = (a, P_M, OUT, b)
    exp = (b, P_M, IN, c)                    # department <- its members
    tys = (a, TYPE, OUT, b)                  # student -> its type ids
    tk = (a, P_TK, OUT, b)
    q7 = [(b, TYPE, OUT, T_C), (b, P_TCH, IN, a)]
    return {
        "tail": _plan([s0, tk] + q7, 2),                  # forward-map FN_EQ
        "tail-k2k": _plan([s0, tk, (b, P_TCH, IN, a)], 2),
        "tail-append": _plan([s0, tk] + q7 + [(b, P_NM, OUT, c)], 3),
        "tail-type-append": _plan([s0, tk, (b, TYPE, OUT, T_X),
                                   (b, P_NM, OUT, c)], 3),
        # 2 input columns (Q7's own shape)
        "tail-nc2": _plan([s0, (a, P_HB, OUT, b), (a, P_TK, OUT, c),
                           (c, TYPE, OUT, T_C), (c, P_TCH, IN, a)], 3),
        # students -> department (functional k2u, steps of its own), then
        # department <- members (CSR expansion) with: FN_EQ through the
        # REVERSED map (subOrgOf IN), EQ (k2c through the reversed-only
        # map) and its empty form (host-resolved constant 0), and the
        # maximum of 8 ops with a ninth pattern left to its own step
        "tail-rev": _plan([sS, mem, (b, P_M, IN, c), (c, P_U, OUT, d),
                           (d, P_SUB, IN, b)], 4),
        "tail-eq": _plan([sS, mem, (b, P_M, IN, c), (c, P_U, OUT, d),
                          (d, P_SUB, IN, D0 + 3)], 4),
        "tail-eq-none": _plan([sS, mem, (b, P_M, IN, c), (c, P_U, OUT, d),
                               (d, P_SUB, IN, D0 + ND)], 4),
        "tail-len8+1": _plan([sS, mem, (b, P_M, IN, c), (c, TYPE, OUT, T_ALL),
                              (c, P_U, OUT, d), (d, TYPE, OUT, T_U),
                              (d, P_SUB, IN, b), (b, TYPE, OUT, T_D),
                              (c, P_M, OUT, b), (c, P_NM2, OUT, e),
                              (e, TYPE, OUT, T_L), (b, TYPE, OUT, T_ANY)], 5),
        # length 5
        "tail-len5": _plan([sS, mem, exp, (c, TYPE, OUT, T_ALL),
                            (c, P_U, OUT, d), (d, TYPE, OUT, T_U),
                            (d, P_SUB, IN, b), (b, TYPE, OUT, T_D)], 4),
        # keep-rates: every edge / exactly one edge of the whole table /
        # one edge of one input row in every 64 (one per writer wave)
        "tail-all": _plan([sS, mem, exp, (c, TYPE, OUT, T_ALL),
                           (c, P_M, OUT, b)], 3),
        "tail-one": _plan([sS, mem, exp, (c, P_ONE, OUT, b),
                           (a, P_ONE, OUT, b)], 3),
        "tail-wave": _plan([sS, mem, exp, (a, P_W, OUT, b),
                            (c, P_ONE, OUT, b)], 3),
        # a column of TYPE IDS (below the vid span of every map and
        # bitmap): expansion over rdf:type OUT, then FN_APPEND / TYPE on
        # that column must miss; the third plan shows the same expansion
        # with a chain on the other column keeps rows
        "tail-fn-outside": _plan([sS, tys, (b, P_M, OUT, c),
                                  (c, TYPE, OUT, T_D)], 3),
        "tail-type-outside": _plan([sS, tys, (a, P_M, OUT, c),
                                    (b, TYPE, OUT, T_D)], 3),
        "tail-typeids": _plan([sS, tys, (a, P_M, OUT, c),
                               (c, TYPE, OUT, T_D)], 3),
        # cut by a non-chainable pattern (forward-map k2c) in the middle
        "tail-cut": _plan([sS, mem, (b, P_M, IN, c), (c, TYPE, OUT, T_ALL),
                           (c, P_U, OUT, d), (c, P_M, OUT, D0 + 1),
                           (d, TYPE, OUT, T_U)], 4),
    }


def _cap_plans():
    """Expansion tails whose chain passes EVERY edge, from 63 start rows:
    far more output rows than the minimum capacity."""
    a, b, c = -1, -2, -3
    return {
        # 63 students x 32/33 members each (thread path, one wave row)
        "cap-members": _plan([(s_type(63), TYPE, IN, a), (a, P_M, OUT, b),
                              (b, P_M, IN, c), (c, TYPE, OUT, T_ALL),
                              (c, P_M, OUT, b)], 3),
        # the professors' course ladder incl. the 700-edge hub: every
        # course has a teacher and every teacher is a professor
        "cap-ladder": _plan([(p_type(63), TYPE, IN, a), (a, P_TK, OUT, b),
                             (b, P_TCH, IN, c),
                             (c, TYPE, OUT, p_type(N_SMALL))], 3),
    }


CAP_PLANS = _cap_plans()


def all_cases():
    """(name, plan) of every plan the file runs."""
    out = list(CAP_PLANS.items())
    for n in ROWS:
        for k, p in tail_plans(p_type(n)).items():
            if k != "tail-nc2" or n in WIDE_ROWS:
                out.append(("%s-n%d" % (k, n), p))
    return out


class Ctx:
    def __init__(self):
        self.triples, self.meta = chain_graph(N_SMALL)
        self.ora = OracleCtx(self.triples)
        self.cases = all_cases()
        self._want = {}

    def want(self, name, plan):
        if name not in self._want:
            r = sort_rows(self.ora.run_query(plan))
            r.setflags(write=False)
            self._want[name] = r
        return self._want[name]


@pytest.fixture(scope="module")
def ctx():
    return Ctx()


# ---------------------------------------------------------------------
# CPU part
# ---------------------------------------------------------------------
def test_oracle_vs_brute(ctx):
    for name, plan in ctx.cases:
        a = ctx.want(name, plan)
        b = sort_rows(ctx.ora.brute_query(plan))
        assert _same(a, b), name


def test_graph_properties(ctx):
    store = wk.Store(ctx.triples)
    assert store.check() == 0
    for p, d in ((P_M, OUT), (P_U, OUT), (P_SUB, OUT), (P_ONE, OUT),
                 (P_W, OUT), (P_NM, OUT), (P_TCH, IN)):
        k, e = store.seg_stats(p, d)
        assert k == e > 0, (p, d)                 # functional
    for p, d in ((P_SUB, IN), (P_TCH, OUT), (P_M, IN)):
        k, e = store.seg_stats(p, d)
        assert 0 < k < e, (p, d)                  # not functional
    k, e = store.seg_stats(P_TK, OUT)
    assert e // k <= 32                           # typeof/chain-fused gate
    k, e = store.seg_stats(P_HB, OUT)
    assert e // k > 32
    n = N_SMALL
    w = lambda k_: len(ctx.want("%s-n%d" % (k_, n), dict(ctx.cases)[
        "%s-n%d" % (k_, n)]))
    assert w("tail-eq-none") == 0
    for k_ in ("tail", "tail-k2k", "tail-append", "tail-type-append",
               "tail-rev", "tail-eq", "tail-len8+1", "tail-cut", "tail-len5",
               "tail-typeids"):
        assert 0 < w(k_), k_
    members = lambda q: len(store.get_triples(int(ctx.meta["D"][q % ND]),
                                              P_M, IN))
    assert w("tail-all") == sum(members(q) for q in range(n))
    assert w("tail-one") == 1 and w("tail-wave") == (n + 63) // 64
    assert w("tail-fn-outside") == 0 and w("tail-type-outside") == 0
    # the capacity plans: every edge passes, 32- and 33-edge rows, and at
    # 64 rows of capacity a 33-edge row of the ladder straddles the end
    for key, plan in CAP_PLANS.items():
        assert len(ctx.want(key, plan)) > 20 * 64, key
    degs = [HUB_DEG if q == HUB else LAD[q % len(LAD)] for q in range(6)]
    assert degs[5] == 33 and sum(degs[:5]) < 64 < sum(degs)
    k, e = store.seg_stats(P_M, IN)
    assert e // k <= 32 and e > 32 * k            # 32- and 33-edge rows
    # the hub's passing edges sit on both sides of the 64-edge chunks
    hub = int(ctx.meta["Pr"][HUB])
    t = ctx.want("tail-n%d" % n, dict(ctx.cases)["tail-n%d" % n])
    lst = store.get_triples(hub, P_TK, OUT)
    pos = sorted(int(np.searchsorted(lst, z)) for y, z in t.tolist() if y == hub)
    # (passing ranks carry from one 64-edge chunk of the wave pass to the next)
    assert len(pos) >= 4 and len({p_ // 64 for p_ in pos}) >= 3


# ---------------------------------------------------------------------
# GPU part
# ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def engines(ctx):
    out = {}
    for name, kv in STORE_ENVS.items():
        with env(**kv):
            out[name] = wk.Engine(wk.GpuStore(wk.Store(ctx.triples), device=0))
    return out


def _rows(eng, plan, path):
    if path == "run_query":
        return sort_rows(eng.run_query(plan))
    eng.submit(plan)
    return sort_rows(eng.fetch_result())


def _check(eng, ctx, name, plan):
    want = ctx.want(name, plan)
    for path in ("run_query", "submit"):
        got = _rows(eng, plan, path)
        assert _same(got, want), (name, path, got.shape, want.shape)
        with env(WK_CHAIN=0):
            ref = _rows(eng, plan, path)
        assert _same(ref, got), (name, path)


@pytest.mark.gpu
@pytest.mark.parametrize("config", list(STORE_ENVS))
def test_plans_exact(ctx, engines, config):
    """Every plan, plain paths, on every store: with hash-only stores and
    without type bitmaps the collector declines and nothing changes."""
    eng = engines[config]
    cases = ctx.cases if config == "default" else \
        [c for c in ctx.cases if c[0].endswith(("-n257", "-n2049", "-n0"))]
    for name, plan in cases:
        _check(eng, ctx, name, plan)


@pytest.mark.gpu
def test_graph_replay(ctx, engines):
    """graph_build + two replays + fetch, per plan shape; a suite capture
    of three plans."""
    eng = engines["default"]
    todo = [c for c in ctx.cases if c[0].endswith(("-n0", "-n65", "-n2049"))]
    for name, plan in todo:
        want = ctx.want(name, plan)
        gid = eng.graph_build(plan)
        for _ in range(2):
            assert eng.graph_run(gid) == len(want), name
            got = sort_rows(eng.fetch_result(plan))
            assert _same(got, want), name
    pick = ["tail-len8+1-n2049", "tail-append-n2049", "tail-nc2-n257"]
    plans = [dict(ctx.cases)[k] for k in pick]
    sid = eng.graph_build_suite(plans)
    for _ in range(2):
        eng.graph_launch(sid)
        eng.sync()
        got = sort_rows(eng.fetch_result(plans[-1]))
        want = ctx.want(pick[-1], plans[-1])
        assert _same(got, want)
    for k, p in zip(pick, plans):
        _check(eng, ctx, k, p)


@pytest.mark.gpu
def test_chain_runs_and_step_api_does_not(ctx):
    """Whole-plan runs take the chain kernels (fewer timed launches than
    with WK_CHAIN=0); the step API keeps one step per pattern: its row
    counts equal WK_CHAIN=0's and the oracle executor's."""
    with env(WK_KERNEL_TIMING=1):
        eng = wk.Engine(wk.Store(ctx.triples), device=0)

    def launches(plan):
        n0 = sum(v["launches"] for v in eng.kernel_stats().values())
        eng.run_query(plan)
        return sum(v["launches"] for v in eng.kernel_stats().values()) - n0

    for key in ("tail-len8+1-n1025", "tail-append-n2049", "tail-typeids-n257",
                "cap-members", "cap-ladder"):
        plan = dict(ctx.cases)[key]
        on = launches(plan)
        with env(WK_CHAIN=0):
            off = launches(plan)
        assert on < off, (key, on, off)

        def steps():
            eng.begin_query(plan)
            seq = []
            while eng.pattern_step < len(plan.patterns):
                n = eng.execute_one_pattern()
                seq.append((eng.pattern_step, n))
            return seq, sort_rows(eng.fetch_result(plan))

        seq_on, rows_on = steps()
        with env(WK_CHAIN=0):
            seq_off, rows_off = steps()
        assert seq_on == seq_off, key
        assert _same(rows_on, ctx.want(key, plan)), key
        assert _same(rows_off, rows_on), key
        ex = OracleExecutor(ctx.ora, plan)
        ora = {}
        while ex.step_no < len(plan.patterns):
            n = ex.step()
            ora[ex.step_no] = n
        # the engine may fuse a typeof filter into its k2u: compare at the
        # pattern indexes it stopped at, and it stops at most one apart
        assert len(seq_on) >= (len(plan.patterns) + 1) // 2, key
        for at, n in seq_on:
            assert ora[at] == n, (key, at, n, ora[at])


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(CAP_PLANS))
def test_capacity_rerun(ctx, engines, key):
    """Expansion tail from a 64-row capacity: the chain's exact count
    exceeds it, so the first run raises S_ERR/S_REQ inside the chain step
    (asserted: the first fetch reports the overflow), the writers clamp
    at `cap` on the thread and on the wave path, the engine grows and the
    re-run is exact."""
    gstore = engines["default"]._store
    plan = CAP_PLANS[key]
    want = ctx.want(key, plan)
    with env(WK_MIN_CAP=64):
        eng = wk.Engine(gstore)
        eng.submit(plan)
        assert eng.fetch_count() < 0, key      # overflowed, capacity grown
        tries = 1
        eng.submit(plan)
        while eng.fetch_count() < 0:
            eng.submit(plan)
            tries += 1
        assert tries <= 3, key
        got = sort_rows(eng.fetch_result())
        assert _same(got, want), key
        eng = wk.Engine(gstore)
        got = sort_rows(eng.run_query(plan))
        assert _same(got, want), key
        eng = wk.Engine(gstore)
        gid = eng.graph_build(plan)
        for _ in range(2):
            assert eng.graph_run(gid) == len(want), key
