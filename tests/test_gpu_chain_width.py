"""Width-sized chain rows and the op-major one-pass filter (DESIGN.md §3
item 3 and 5i).

The batched chain kernels (k_row_chain, k_csr_gather_chain, k_expand_chain)
carry a candidate row as sid_t[4] when the plan's widened row has at most 4
columns, else as sid_t[8]; WK_CHAIN_WIDTH=8 forces the wide instantiation.
k_filter_tpr evaluates the 4 rows of a thread op-major on its plain-gather
paths (type bitmap, PM_EQ, functional map forward / reversed / const);
WK_FILTER_BATCH=0 keeps the row-after-row evaluation.  Every arm must give
the oracle's rows, exactly, as sorted row multisets.

The graph: 2049 subjects A with functional maps to departments (P_G, P_G2,
every subject), to a label of their own (P_H, absent for q % 3 == 0) and an
edge ladder P_E into a course pool (0 .. 40 edges, so rows of > 32 edges and
rows of <= 32 meet in one table); courses map to labels (P_CL, absent for
m % 5 == 0), labels back to subjects (P_BACK: the own subject for even
labels, the next one for odd), departments to E (P_DH), E to F (P_EH): six
appends behind one expansion reach ROW_MAX = 8 columns.  D[0] has two types
(a multi-type vertex under a TYPE op), P_R is functional only in the IN
direction (the host-resolved PM_EQ / CH_EQ form), and type ids as keys lie
below every map and bitmap span.  Start sets of 1, 63, 64, 65, 1023, 1024,
1025 and 2049 rows sit on both sides of the 64-lane wave and the 1024-row
tile of k_row_chain and k_filter_tpr.

A verify-only filter of a capture checks an immutable store with an exact
test, so by itself it cannot miss in a replay.  The guard is therefore
exercised with the mechanisms the engine has for that: a store without type
bitmaps, where the optimistic expansion in front of the verify-only filters
misses on a multi-typed entity (the chain plans of
test_graph_replay_bookkeeping), and WK_FORCE_EMPTY_HINT, which makes the
replay's emptiness guard fail.  Either way the sticky error is raised, the
replay is discarded and the plain path gives the oracle rows.

CPU part (unmarked): oracle == brute for every plan, and the oracle alone
gives the none / all / mixed keep rates the GPU cases rely on.
"""
import numpy as np
import pytest

import wukong_amd as wk
from wukong_amd import Plan
from tests import test_graph_replay_bookkeeping as R
from tests.oracle_util import OracleCtx, sort_rows
from tests.synth_graph import B, IN, OUT, TYPE, env

NA = 2049
ROWS = [1, 63, 64, 65, 1023, 1024, 1025, NA]
NCP, ND, NE, NF = 211, 16, 4, 2
DEGS = [0, 1, 3, 4, 5, 33, 2, 40, 32]      # P_E degree of subject q: q % 9

(P_G, P_G2, P_H, P_E, P_CL, P_BACK, P_DH, P_EH, P_R) = range(2, 11)
T_D, T_X, T_C1, T_HALF, T_NONE, T_L = range(20, 26)
T_R0 = 40                                   # T_R0 + i: first ROWS[i] subjects

STORE_ENVS = {"default": {}, "notbm": dict(WK_TBM=0)}
ARMS = {
    "new": {},
    "wide": dict(WK_CHAIN_WIDTH=8),
    "rowwise": dict(WK_FILTER_BATCH=0),
    "unfused": dict(WK_CHAIN=0),            # every pattern a step of its own
    "unfused-rowwise": dict(WK_CHAIN=0, WK_FILTER_BATCH=0),
}


def r_type(n):
    return T_R0 + ROWS.index(n)


def width_graph():
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

    A, C, L, D, E, F, K = (take(NA), take(NCP), take(NA), take(ND), take(NE),
                           take(NF), take(3))
    q = np.arange(NA)
    m = np.arange(NCP)
    add(A, P_G, D[q % ND])
    add(A, P_G2, D[(q * 3) % ND])
    add(A[q % 3 != 0], P_H, L[q[q % 3 != 0]])
    add(L, P_BACK, A[np.where(q % 2 == 0, q, (q + 1) % NA)])
    for i in range(NA):
        d = DEGS[i % len(DEGS)]
        if d:
            add(A[i], P_E, C[(i * 7 + np.arange(d)) % NCP])
    add(C[m % 5 != 0], P_CL, L[m[m % 5 != 0]])
    add(D, P_DH, E[np.arange(ND) % NE])
    add(E, P_EH, F[np.arange(NE) % NF])
    add(A[[5, 5, 6]], P_R, K)               # functional in the IN direction
    add(D, TYPE, T_D)
    add(D[0], TYPE, T_X)                    # multi-type vertex
    add(C[m % 2 == 0], TYPE, T_C1)
    add(A[q % 2 == 0], TYPE, T_HALF)
    add(L, TYPE, T_L)
    add(K[0], TYPE, T_NONE)                 # a type no subject / course is in
    for n in ROWS:
        add(A[:n], TYPE, r_type(n))
    meta = dict(A=A, C=C, L=L, D=D, E=E, F=F, K=K)
    return np.unique(np.concatenate(trip).astype(np.uint32), axis=0), meta


def _plan(pats, nvars):
    return Plan(pats, nvars=nvars,
                required_vars=[-(v + 1) for v in range(nvars)])


def plans(n, meta):
    a, b, c, d, e, f, g, h = range(-1, -9, -1)
    s0 = (r_type(n), TYPE, IN, a)
    D, K = meta["D"], meta["K"]
    out = {
        # ---- row pass, out_cols 2, 3, 4, 5, 8 ---------------------------
        "rp2": _plan([s0, (a, P_G, OUT, b), (b, TYPE, OUT, T_D)], 2),
        "rp3": _plan([s0, (a, P_G, OUT, b), (a, P_G2, OUT, c),
                      (b, TYPE, OUT, T_D)], 3),
        # FN_EQ reads the column appended before it; absent append keys
        "rp4": _plan([s0, (a, P_G, OUT, b), (a, P_H, OUT, c),
                      (c, P_BACK, OUT, a), (a, P_G2, OUT, d)], 4),
        "rp5": _plan([s0, (a, P_G, OUT, b), (a, P_G2, OUT, c),
                      (a, P_H, OUT, d), (b, P_DH, OUT, e)], 5),
        "rp8": _plan([s0, (a, P_G, OUT, b), (a, P_G2, OUT, c),
                      (a, P_H, OUT, d), (b, P_DH, OUT, e), (c, P_DH, OUT, f),
                      (d, P_BACK, OUT, g), (e, P_EH, OUT, h)], 8),
        # keep rates of the row pass: all / none / mixed
        "rp-all": _plan([s0, (a, P_G, OUT, b), (a, P_G2, OUT, c)], 3),
        "rp-none": _plan([s0, (a, P_G, OUT, b), (b, TYPE, OUT, T_NONE)], 2),
        "rp-mixed": _plan([s0, (a, P_G, OUT, b), (a, TYPE, OUT, T_HALF)], 2),
        # TYPE on the multi-type vertex; EQ (reversed map, host-resolved)
        "rp-multi": _plan([s0, (a, P_G, OUT, b), (b, TYPE, OUT, T_X)], 2),
        "rp-eq": _plan([s0, (a, P_G, OUT, b), (a, P_R, OUT, int(K[0]))], 2),
        # the row pass in one query with an expansion that overflows a
        # small capacity
        "rp-cap": _plan([s0, (a, P_G, OUT, b), (b, TYPE, OUT, T_D),
                         (a, P_E, OUT, c)], 3),
        # ---- one-pass filter paths --------------------------------------
        "f-type-all": _plan([s0, (a, TYPE, OUT, r_type(NA))], 1),
        "f-type-none": _plan([s0, (a, TYPE, OUT, T_NONE)], 1),
        "f-type-mixed": _plan([s0, (a, TYPE, OUT, T_HALF)], 1),
        "f-k2k-fwd": _plan([s0, (a, P_G, OUT, b), (a, P_G2, OUT, b)], 2),
        # subject b is column 1; (P_G, IN) is not functional: fn_swap
        "f-k2k-rev": _plan([s0, (a, P_G2, OUT, b), (b, P_G, IN, a)], 2),
        "f-const": _plan([s0, (a, P_G, OUT, int(D[3]))], 1),
        "f-const-col1": _plan([s0, (a, P_G, OUT, b),
                               (b, P_DH, OUT, int(meta["E"][1]))], 2),
        "f-eq": _plan([s0, (a, P_R, OUT, int(K[0]))], 1),
        "f-eq-none": _plan([s0, (a, P_R, OUT, int(D[0]))], 1),
    }
    return out


def exp_plans(n, meta):
    """Expansion-fused chains: NC input columns + the edge value."""
    a, b, c, d, e, f, g, h = range(-1, -9, -1)
    s0 = (r_type(n), TYPE, IN, a)
    ex = (a, P_E, OUT, b)
    ops = [(b, P_CL, OUT, c), (c, P_BACK, OUT, d), (d, P_G, OUT, e),
           (d, P_G2, OUT, f), (e, P_DH, OUT, g), (g, P_EH, OUT, h)]
    out = {
        "ex2": _plan([s0, ex, (b, TYPE, OUT, T_C1)], 2),
        "ex2-none": _plan([s0, ex, (b, TYPE, OUT, T_NONE)], 2),
        "ex3": _plan([s0, ex, (b, TYPE, OUT, T_C1), ops[0]], 3),
        "ex4": _plan([s0, ex] + ops[:2], 4),
        "ex5": _plan([s0, ex] + ops[:3], 5),
        "ex8": _plan([s0, ex] + ops, 8),
        # FN_EQ on the appended label's back pointer; EQ on the input column
        "ex-fneq": _plan([s0, ex, ops[0], (c, TYPE, OUT, T_L),
                          (a, P_H, OUT, c)], 3),
        "ex-eq": _plan([s0, ex, (a, P_R, OUT, int(meta["K"][2])),
                        (b, TYPE, OUT, T_C1)], 2),
        # type ids as keys: below every span, every candidate drops
        "ex-typeids": _plan([s0, (a, TYPE, OUT, b), (b, P_CL, OUT, c),
                             (c, TYPE, OUT, T_L)], 3),
        # NC = 3 + the edge fills the narrow bucket; NC = 4 is wide
        "ex-nc3": _plan([s0, (a, P_G, OUT, c), (a, P_G2, OUT, d), ex,
                         (b, TYPE, OUT, T_C1)], 4),
        "ex-nc4": _plan([s0, (a, P_G, OUT, c), (a, P_G2, OUT, d),
                         (a, P_H, OUT, e), ex, (b, TYPE, OUT, T_C1)], 5),
    }
    return out


EXP_ROWS = [1, 65, 1025, NA]


def _same(got, want):
    if len(got) == 0 or len(want) == 0:
        return len(got) == len(want)
    return got.shape == want.shape and np.array_equal(got, want)


class Ctx:
    def __init__(self):
        self.triples, self.meta = width_graph()
        self.ora = OracleCtx(self.triples)
        self.cases = {}
        for n in ROWS:
            for k, p in plans(n, self.meta).items():
                self.cases["%s-n%d" % (k, n)] = p
        for n in EXP_ROWS:
            for k, p in exp_plans(n, self.meta).items():
                self.cases["%s-n%d" % (k, n)] = p
        self._want = {}

    def want(self, name):
        if name not in self._want:
            r = sort_rows(self.ora.run_query(self.cases[name]))
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
    for name, plan in ctx.cases.items():
        if name.endswith(("-n65", "-n1025")):
            assert _same(ctx.want(name),
                         sort_rows(ctx.ora.brute_query(plan))), name


def test_graph_properties(ctx):
    store = wk.Store(ctx.triples)
    assert store.check() == 0
    A, D = ctx.meta["A"], ctx.meta["D"]
    for p in (P_G, P_G2, P_H, P_CL, P_BACK, P_DH, P_EH):
        k, e = store.seg_stats(p, OUT)
        assert k == e > 0, p                          # functional
    k, e = store.seg_stats(P_R, OUT)
    assert 0 < k < e                                  # OUT is not functional
    k, e = store.seg_stats(P_R, IN)
    assert k == e == 3                                # IN is
    k, e = store.seg_stats(P_G, IN)
    assert 0 < k < e
    k, e = store.seg_stats(P_E, OUT)
    assert 0 < k < e and e // k <= 32                 # chain-fused gate
    degs = {len(store.get_triples(int(A[i]), P_E, OUT)) for i in range(9)}
    assert degs == set(DEGS) and max(degs) > 32
    assert sorted(store.get_triples(int(D[0]), TYPE, OUT)) == [T_D, T_X]
    for n in ROWS:
        w = lambda k_: len(ctx.want("%s-n%d" % (k_, n)))
        assert len(store.get_index(r_type(n), IN)) == n
        # none / all / mixed, for the row pass and for the filter
        assert w("rp-all") == n == w("f-type-all") == w("rp2")
        assert w("rp-none") == 0 == w("f-type-none") == w("f-eq-none")
        assert w("rp-mixed") == (n + 1) // 2 == w("f-type-mixed")
        assert w("rp-multi") == (n + ND - 1) // ND    # subjects of D[0]
        assert w("f-k2k-fwd") == (n + 7) // 8 == w("f-k2k-rev")
        assert w("f-const") == (n + ND - 4) // ND
        assert w("rp-eq") == w("f-eq") == (1 if n > 5 else 0)
        if n >= 63:
            assert 0 < w("rp4") < w("rp5") < n        # absent keys, FN_EQ
            assert w("rp8") == w("rp5") and w("rp3") == n
            assert 0 < w("f-const-col1") < n
            assert w("rp-cap") > 4 * n
    for n in EXP_ROWS:
        w = lambda k_: len(ctx.want("%s-n%d" % (k_, n)))
        assert w("ex2-none") == 0 == w("ex-typeids")
        if n > 1:
            assert 0 < w("ex8") == w("ex5") == w("ex4")
            assert 0 < w("ex3") < w("ex4") and w("ex3") < w("ex2")
            assert 0 < w("ex-fneq") < w("ex3")
            assert 0 < w("ex-nc3") and 0 < w("ex-nc4") < w("ex-nc3")
            assert w("ex-eq") == 1                    # A[6]: 2 edges, 1 even
            # a row with edges none of which passes, and a > 32-edge row
            # that keeps some: both classes meet in one table
            ex2 = ctx.want("ex2-n%d" % n)
            kept = set(ex2[:, 0].tolist())
            assert int(A[1]) not in kept              # one edge, odd course
            assert int(A[7]) in kept and int(A[5]) in kept
    assert len(ctx.want("ex2-n1")) == 0               # A[0] has no edge


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


def _check_arms(eng, ctx, name, arms, paths=("run_query",)):
    plan, want = ctx.cases[name], ctx.want(name)
    for arm in arms:
        with env(**ARMS[arm]):
            for path in paths:
                got = _rows(eng, plan, path)
                assert _same(got, want), (name, arm, path, got.shape,
                                          want.shape)


@pytest.mark.gpu
@pytest.mark.parametrize("config", list(STORE_ENVS))
def test_row_pass_and_expansion_widths(ctx, engines, config):
    """Both width arms (and the unfused engine) against the oracle, for
    every row-pass and expansion-fused plan at every row count."""
    eng = engines[config]
    for name in ctx.cases:
        if name.startswith(("rp", "ex")):
            _check_arms(eng, ctx, name, ("new", "wide", "unfused"))


@pytest.mark.gpu
@pytest.mark.parametrize("config", list(STORE_ENVS))
def test_filter_paths(ctx, engines, config):
    """k_filter_tpr batched and row-after-row, fused engine and one step
    per pattern; without bitmaps the typeof filter is on the per-row path
    either way and must still be right."""
    eng = engines[config]
    for name in ctx.cases:
        if name.startswith(("f-", "rp-mixed", "rp-eq")):
            _check_arms(eng, ctx, name,
                        ("new", "rowwise", "unfused", "unfused-rowwise"))


@pytest.mark.gpu
def test_submit_path(ctx, engines):
    eng = engines["default"]
    for name in ctx.cases:
        if name.endswith(("-n1", "-n1025")):
            _check_arms(eng, ctx, name, ("new", "wide", "unfused-rowwise"),
                        paths=("submit",))


@pytest.mark.gpu
@pytest.mark.parametrize("arm", ["new", "wide", "rowwise", "unfused"])
def test_captures_equal_submit(ctx, engines, arm):
    """graph_build / graph_run and graph_build_suite replays of the same
    plans give the rows of submit."""
    eng = engines["default"]
    names = [k for k in ctx.cases if k.endswith(("-n65", "-n1025"))]
    with env(**ARMS[arm]):
        for name in names:
            plan, want = ctx.cases[name], ctx.want(name)
            gid = eng.graph_build(plan)
            for _ in range(2):
                assert eng.graph_run(gid) == len(want), (arm, name)
                got = sort_rows(eng.fetch_result(plan))
                assert _same(got, want), (arm, name)
        for last in ("rp4-n1025", "ex8-n1025", "f-k2k-rev-n1025",
                     "f-type-mixed-n1025"):
            pick = ["rp8-n65", "ex-nc3-n1025", "f-const-n1025", last]
            suite = [ctx.cases[k] for k in pick]
            sid = eng.graph_build_suite(suite)
            for _ in range(2):
                eng.graph_launch(sid)
                eng.sync()
                got = sort_rows(eng.fetch_result(suite[-1]))
                assert _same(got, ctx.want(last)), (arm, last)
        for name in names[:6]:
            _check_arms(eng, ctx, name, (arm,), paths=("submit",))


@pytest.mark.gpu
@pytest.mark.parametrize("arm", ["new", "rowwise"])
@pytest.mark.parametrize("store", ["notbm", "default"])
def test_guard_miss_with_verify_only_filters(arm, store):
    """Captured plans whose filters run verify-only (the warm pass saw no
    drop), with a multi-typed entity in the optimistic expansion in front
    of or behind them: without type bitmaps the replay is discarded by the
    sticky error, never wrong, and the plain path is exact.  Then a forced
    wrong emptiness hint: the replay raises, the re-run is exact."""
    triples, meta = R.chain_graph()
    ora = OracleCtx(triples)
    with env(**STORE_ENVS[store]):
        eng = wk.Engine(wk.Store(triples), device=0)
    with env(**ARMS[arm]):
        for where in ("first", "last", "none"):
            plan = R.chain_plan(where, 1025, meta["c0"])
            want = sort_rows(ora.run_query(plan))
            assert len(want) > 1025
            R._check_replays(eng, plan, want, (arm, store, where),
                             may_miss=store != "default" and where != "none")
        plan = R.chain_plan("none", 1023, meta["c0"])
        want = sort_rows(ora.run_query(plan))
        with env(WK_FORCE_EMPTY_HINT=0):
            gid = eng.graph_build(plan)
        for _ in range(2):
            with pytest.raises(OverflowError):
                eng.graph_run(gid)
            got = sort_rows(eng.run_query(plan))
            assert _same(got, want), (arm, store)
        gid = eng.graph_build(plan)
        assert eng.graph_run(gid) == len(want)


@pytest.mark.gpu
@pytest.mark.parametrize("arm", ["new", "wide"])
@pytest.mark.parametrize("key", ["rp-cap-n1025", "ex-nc3-n1025", "ex8-n1025"])
def test_capacity_rerun(ctx, engines, arm, key):
    """A 64-row capacity overflows in the expansion (in front of the row
    pass, or inside the chain step): the engine grows, the re-run is exact
    at both widths."""
    gstore = engines["default"]._store
    plan, want = ctx.cases[key], ctx.want(key)
    assert len(want) > 4 * 64
    with env(WK_MIN_CAP=64, **ARMS[arm]):
        eng = wk.Engine(gstore)
        eng.submit(plan)
        assert eng.fetch_count() < 0, key
        tries = 1
        eng.submit(plan)
        while eng.fetch_count() < 0:
            eng.submit(plan)
            tries += 1
        assert tries <= 3, key
        assert _same(sort_rows(eng.fetch_result()), want), key
        eng = wk.Engine(gstore)
        assert _same(sort_rows(eng.run_query(plan)), want), key
        eng = wk.Engine(gstore)
        gid = eng.graph_build(plan)
        for _ in range(2):
            assert eng.graph_run(gid) == len(want), key
