"""k_filter_expr and its placement: FILTER with =, !=,
bound, &&, ||, ! on the GPU, through every entry point.

The graph below is built for this file: one start set per row count
(through the type index and through a constant's edge list, both
zero-copy views), 1:1 columns that select the keep patterns of the
compaction (alternating rows, lane 0 of each wave, one whole wave, the
last row), an OPTIONAL pair with BLANK rows, and a small-degree
expansion with a typed, functional tail for the fused steps.

The oracle has no FILTER: the expected rows of every case are
tests/filter_ref.py over the oracle's table of the same plan without the
filter.  All comparisons are exact sorted-row equality.

CPU part (unmarked): every case is well-formed for the oracle and the
data-dependent ones keep some rows and drop some.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import wukong_amd as wk
from wukong_amd import Plan
from tests import filter_ref
from tests.oracle_util import OracleCtx, sort_rows
from tests.synth_graph import B, IN, OUT, TYPE, env

ROWS = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049]
N = 2049
BIG = 2048 * 1024 + 1025           # second trip of the grid-stride loop
P_SET, P_ALT, P_LANE, P_WAVE, P_K7, P_OPT, P_OPT2, P_EXP, P_Q = range(2, 11)
T_M, T_BIG = 20, 21
T_S0 = 40                          # T_S0 + i: first ROWS[i] row entities
NM = 257
LAD = [0, 1, 2, 3, 5, 33, 2, 1]    # P_EXP degrees (avg < 32: CSR + fusions)
X, Y, Z, W, U = -1, -2, -3, -4, -5

STORE_ENVS = {"default": {}, "hash": dict(WK_FN=0, WK_CSR=0, WK_TBM=0)}


def filter_graph():
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

    R, V, K, Wv = take(N), take(2), take(64), take(N // 64 + 1)
    O, M, Qv, H = take(N), take(NM), take(NM), take(len(ROWS))
    i = np.arange(N)
    for k, n in enumerate(ROWS):
        if n:
            add(R[:n], TYPE, T_S0 + k)         # index start
            add(H[k], P_SET, R[:n])            # constant start
    add(R, P_ALT, V[i % 2])
    add(R, P_LANE, K[i % 64])
    add(R, P_WAVE, Wv[i // 64])
    add(R, P_K7, K[i % 7])
    # OPTIONAL pair: both columns bound iff i % 6 == 0, equal iff i % 12 == 0
    add(R[i % 3 == 0], P_OPT, O[i[i % 3 == 0]])
    ev = i[i % 2 == 0]
    add(R[ev], P_OPT2, np.where(ev % 12 == 0, O[ev], O[(ev + 1) % N]))
    for q in range(N):
        deg = LAD[q % len(LAD)]
        if deg:
            add(R[q], P_EXP, M[(3 * q + 5 * np.arange(deg)) % NM])
    m = np.arange(NM)
    add(M[m % 4 != 1], TYPE, T_M)
    add(M[m % 5 != 0], P_Q, Qv[m[m % 5 != 0]])
    meta = dict(R=R, V=V, K=K, Wv=Wv, O=O, M=M, Qv=Qv, H=H)
    return np.concatenate(trip).astype(np.uint32), meta


def _start(g, kind, n):
    k = ROWS.index(n)
    if kind == "i2u":
        return (T_S0 + k, TYPE, IN, X)
    return (int(g["H"][k]), P_SET, OUT, X)


COLS = [(X, P_ALT, OUT, Y), (X, P_LANE, OUT, Z), (X, P_WAVE, OUT, W),
        (X, P_K7, OUT, U)]


def _plan(pats, nvars, flt, **kw):
    return Plan(pats, nvars=nvars,
                required_vars=[-(v + 1) for v in range(nvars)],
                filters=flt, **kw)


def _or_all(leaves):
    e = leaves[0]
    for leaf in leaves[1:]:
        e = ("or", e, leaf)
    return e


def keep_filters(g, n, width):
    """name -> filter list: the keep patterns and expression forms that
    a table of `width` columns can express."""
    R, V, K, Wv = g["R"], g["V"], g["K"], g["Wv"]
    last = int(R[max(n, 1) - 1])
    f = {"all": [("eq", X, X)], "none": [("ne", X, X)],
         "last": [("eq", last, X)],                      # constant on the left
         "not-last": [("ne", X, last)]}
    if width == 1:
        # 16 leaves + 15 ORs + NOT: a 32-node program (drops the even
        # rows below 32)
        f["prog32"] = [("not", _or_all([("eq", X, int(R[2 * j]))
                                       for j in range(16)]))]
        return f
    f["bound"] = [("bound", Y)]
    f["alt"] = [("eq", Y, int(V[0]))]
    f["alt-not"] = [("not", ("eq", Y, int(V[0])))]
    f["var-ne-var"] = [("ne", Y, X)]                     # always true
    if width == 2:
        return f
    f["lane0"] = [("eq", Z, int(K[0]))]
    f["wave1"] = [("eq", W, int(Wv[1]))]
    f["var-eq-var"] = [("eq", Z, U)]
    f["and"] = [("and", ("eq", Y, int(V[1])), ("ne", Z, int(K[1])))]
    f["or"] = [("or", ("eq", W, int(Wv[0])), ("eq", U, int(K[3])))]
    f["clauses"] = [("ne", X, int(R[0])), ("eq", Y, int(V[0])),
                    ("not", ("eq", Z, int(K[2])))]
    f["depth5"] = [("or", ("and", ("eq", Y, int(V[0])),
                           ("not", ("or", ("eq", Z, int(K[0])),
                                    ("and", ("ne", W, int(Wv[0])),
                                     ("not", ("eq", U, int(K[2]))))))),
                    ("eq", X, last))]
    return f


def sweep_cases(g):
    out = {}
    for kind in ("i2u", "c2u"):
        for n in ROWS:
            for width in (1, 2, 5):
                pats = [_start(g, kind, n)] + COLS[:width - 1]
                for name, flt in keep_filters(g, n, width).items():
                    out["%s-n%d-w%d-%s" % (kind, n, width, name)] = \
                        _plan(pats, width, flt)
    return out


def group_cases(g):
    """OPTIONAL / UNION plans: BLANK semantics, branch-born variables."""
    O, V, K = g["O"], g["V"], g["K"]
    opt = [(X, P_OPT, OUT, Y), (X, P_OPT2, OUT, Z)]
    out = {}
    for n in (65, 1025):
        s = _start(g, "i2u", n)
        for name, flt in (
                ("bound", [("bound", Y)]),
                ("unbound", [("not", ("bound", Y))]),
                ("ne-const", [("ne", Y, int(O[6]))]),    # blank != c: true
                ("eq-vars", [("eq", Y, Z)]),             # blank == blank
                ("main+opt", [("ne", X, int(g["R"][0])),
                              ("or", ("bound", Z), ("eq", X, int(g["R"][1])))])):
            out["opt-n%d-%s" % (n, name)] = _plan([s], 3, flt, optional=opt)
        un = [[(X, P_ALT, OUT, Y)], [(X, P_LANE, OUT, Y)]]
        out["union-n%d" % n] = _plan(
            [s], 2, [("or", ("eq", Y, int(V[0])), ("eq", Y, int(K[3])))],
            unions=un)
        out["union-main-n%d" % n] = _plan(
            [s, (X, P_WAVE, OUT, Z)], 3,
            [("ne", Z, int(g["Wv"][0])), ("ne", Y, int(V[1]))],
            unions=[[(X, P_ALT, OUT, Y)], [(X, P_K7, OUT, Y)]])
    return out


def placement_cases(g):
    """Filters behind fused steps and in front of expansions."""
    R, M, Qv, K = g["R"], g["M"], g["Qv"], g["K"]
    A, Bq = -2, -3
    out = {}
    for n in (65, 2049):
        s = _start(g, "i2u", n)
        exp = (X, P_EXP, OUT, A)
        # 5i: expansion + [typeof, fn append] as one step; the filter on
        # the appended variable lands behind it, the one on ?x in front
        out["chain-n%d" % n] = _plan(
            [s, exp, (A, TYPE, OUT, T_M), (A, P_Q, OUT, Bq)], 3,
            [("ne", Bq, int(Qv[7])), ("ne", X, int(R[3]))])
        # 5h: expansion + typeof in one step, filter on its new column
        out["tf-n%d" % n] = _plan(
            [s, exp, (A, TYPE, OUT, T_M)], 2,
            [("or", ("eq", A, int(M[2])), ("eq", A, int(M[8])))])
        # filter in front of an expansion, dropping 63 rows of 64
        out["pre-exp-n%d" % n] = _plan(
            [s, (X, P_LANE, OUT, A), (X, P_EXP, OUT, Bq)], 3,
            [("eq", A, int(K[5]))])
    # captured plan whose tail is empty: the filter behind pattern 1
    # drops every row; the one on ?w would run inside the skipped tail
    out["empty-tail"] = _plan([_start(g, "i2u", 257)] + COLS[:3], 4,
                              [("ne", Y, Y), ("bound", W)])
    # small start, then an expansion far beyond a 64-row capacity
    out["cap"] = _plan([_start(g, "i2u", 63), (X, P_EXP, OUT, A)], 2,
                       [("ne", X, int(R[5]))])
    return out


class Ctx:
    def __init__(self):
        self.triples, self.g = filter_graph()
        self.ora = OracleCtx(self.triples)
        self.cases = {}
        self.cases.update(sweep_cases(self.g))
        self.cases.update(group_cases(self.g))
        self.cases.update(placement_cases(self.g))
        self._want, self.stats = {}, {}

    def want(self, name):
        if name not in self._want:
            st = {}
            r = sort_rows(filter_ref.expected(self.ora, self.cases[name], st))
            r.setflags(write=False)
            self._want[name], self.stats[name] = r, st
        return self._want[name]


@pytest.fixture(scope="module")
def ctx():
    return Ctx()


def _same(got, want):
    if len(got) == 0 or len(want) == 0:
        return len(got) == len(want)
    return got.shape == want.shape and np.array_equal(got, want)


# ---------------------------------------------------------------------
# CPU part
# ---------------------------------------------------------------------
def test_cases_are_not_vacuous(ctx):
    """Row counts of the reference before/after each filter."""
    for name in ctx.cases:
        ctx.want(name)
    st = ctx.stats
    for kind in ("i2u", "c2u"):
        for n in ROWS:
            for w in (1, 2, 5):
                pre = "%s-n%d-w%d-" % (kind, n, w)
                assert st[pre + "all"]["before"] == n
                assert st[pre + "all"]["after"] == n
                assert st[pre + "none"]["after"] == 0
                assert st[pre + "last"]["after"] == min(n, 1)
                assert st[pre + "not-last"]["after"] == n - min(n, 1)
            assert st["%s-n%d-w1-prog32" % (kind, n)]["after"] == \
                n - len(range(0, min(n, 32), 2))
            pre = "%s-n%d-w5-" % (kind, n)
            assert st[pre + "alt"]["after"] == (n + 1) // 2
            assert st[pre + "alt-not"]["after"] == n // 2
            assert st[pre + "lane0"]["after"] == (n + 63) // 64
            assert st[pre + "wave1"]["after"] == max(0, min(n, 128) - 64)
            assert st[pre + "var-ne-var"]["after"] == n
            if n >= 255:
                for k in ("var-eq-var", "and", "or", "clauses", "depth5"):
                    assert 0 < st[pre + k]["after"] < n, (pre, k)
    for name in list(group_cases(ctx.g)) + list(placement_cases(ctx.g)):
        if name == "empty-tail":
            assert st[name]["after"] == 0 < st[name]["before"]
        else:
            assert 0 < st[name]["after"] < st[name]["before"], (name, st[name])
    # rows with both OPTIONAL columns blank pass `?y = ?z`
    t = ctx.want("opt-n1025-eq-vars")
    blank = (t[:, 1] == filter_ref.BLANK) & (t[:, 2] == filter_ref.BLANK)
    assert blank.any() and (~blank).any()
    assert (ctx.want("opt-n1025-ne-const")[:, 1] == filter_ref.BLANK).any()


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


def _unfiltered_ok(eng, ctx, name):
    """The same plan without its filter still equals the oracle (the
    store's edge list behind a zero-copy start is intact)."""
    bare = filter_ref.unfiltered(ctx.cases[name])
    assert _same(sort_rows(eng.run_query(bare)),
                 sort_rows(ctx.ora.run_query(bare))), name


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["i2u", "c2u"])
def test_sweep_run_query(ctx, engines, kind):
    """Row counts x widths x keep patterns x expression forms; non-blind
    and blind.  Filters on ?x alone run straight on the zero-copy view."""
    eng = engines["default"]
    names = [k for k in sweep_cases(ctx.g) if k.startswith(kind)]
    for name in names:
        want = ctx.want(name)
        got = sort_rows(eng.run_query(ctx.cases[name]))
        assert _same(got, want), (name, got.shape, want.shape)
        if name.endswith(("-none", "-alt", "-last", "-prog32")):
            assert eng.run_query_count(ctx.cases[name]) == len(want), name
            _unfiltered_ok(eng, ctx, name)


@pytest.mark.gpu
def test_second_grid_trip():
    """2048 * 1024 + 1025 rows, one column: the last tiles belong to the
    second trip of the grid-stride loop."""
    ids = np.arange(B, B + BIG, dtype=np.uint32)
    trip = np.stack([ids, np.full(BIG, TYPE, np.uint32),
                     np.full(BIG, T_BIG, np.uint32)], axis=1)
    a, b = int(ids[2048 * 1024 + 3]), int(ids[-1])
    flt = [("not", ("or", ("eq", X, a), ("eq", X, b)))]
    plan = Plan([(T_BIG, TYPE, IN, X)], 1, [X], filters=flt)
    want = ids[filter_ref.keep_mask(ids.reshape(-1, 1), flt)]
    assert len(want) == BIG - 2
    eng = wk.Engine(wk.Store(trip), device=0)
    got = np.sort(eng.run_query(plan).ravel())
    assert np.array_equal(got, want)
    assert eng.run_query_count(plan) == BIG - 2


@pytest.mark.gpu
def test_groups_blank_semantics(ctx, engines):
    """OPTIONAL (bound, !bound, BLANK != c, BLANK == BLANK) and UNION
    (branch-born variable): the reference position, after the groups;
    conjuncts on main-BGP variables alone are still pushed down."""
    for cfg, eng in engines.items():
        for name in group_cases(ctx.g):
            want = ctx.want(name)
            for push in (1, 0):
                with env(WK_FILTER_PUSHDOWN=push):
                    got = sort_rows(eng.run_query(ctx.cases[name]))
                    assert _same(got, want), (cfg, name, push)
                    assert eng.run_query_count(ctx.cases[name]) == len(want)


ENTRY = ["i2u-n0-w5-alt", "i2u-n1-w1-last", "c2u-n65-w2-alt",
         "i2u-n257-w5-depth5", "c2u-n1025-w5-clauses", "i2u-n2049-w1-prog32",
         "i2u-n2049-w5-lane0", "chain-n2049", "tf-n2049", "pre-exp-n2049",
         "empty-tail"]


@pytest.mark.gpu
def test_entry_points(ctx, engines):
    """submit + fetch_count / fetch_result, graph_build + two replays, a
    suite capture mixed with unfiltered plans."""
    eng = engines["default"]
    for name in ENTRY:
        plan, want = ctx.cases[name], ctx.want(name)
        eng.submit(plan)
        assert eng.fetch_count() == len(want), name
        assert _same(sort_rows(eng.fetch_result()), want), name
        gid = eng.graph_build(plan)
        for _ in range(2):
            assert eng.graph_run(gid) == len(want), name
            assert _same(sort_rows(eng.fetch_result(plan)), want), name
    pick = ["chain-n2049", "i2u-n257-w5-depth5", "empty-tail",
            "c2u-n1025-w5-clauses"]
    plans = []
    for name in pick:
        plans += [filter_ref.unfiltered(ctx.cases[name]), ctx.cases[name]]
    sid = eng.graph_build_suite(plans)
    for _ in range(2):
        eng.graph_launch(sid)
        eng.sync()
        assert _same(sort_rows(eng.fetch_result(plans[-1])),
                     ctx.want(pick[-1]))
    for name in pick:
        assert _same(sort_rows(eng.run_query(ctx.cases[name])), ctx.want(name))


@pytest.mark.gpu
def test_no_silent_ignore(ctx, engines):
    """Paths that cannot evaluate a filter refuse the plan; malformed
    programs and never-bound variables are WK_ERR_PLAN."""
    eng = engines["default"]
    g = ctx.g
    tmpl = _plan([_start(g, "c2u", 65), (X, TYPE, OUT, T_S0 + 4)], 1,
                 [("ne", X, int(g["R"][0]))])
    with pytest.raises(ValueError):
        eng.submit_plan_batch(tmpl, [int(g["H"][4])])
    # the same two-pattern shape takes the per-pattern path, not k_light2
    want = sort_rows(filter_ref.expected(ctx.ora, tmpl))
    assert len(want) == 64
    eng.submit(tmpl)
    assert _same(sort_rows(eng.fetch_result()), want)
    assert _same(sort_rows(eng.run_query(tmpl)), want)
    # a variable that no pattern binds
    lost = Plan([_start(g, "i2u", 65)], 2, [X], filters=[("ne", X, Y)])
    with pytest.raises(RuntimeError):
        eng.run_query(lost)
    with pytest.raises(RuntimeError):
        eng.begin_query(lost)
    # malformed programs straight at the ABI
    good = _plan([_start(g, "i2u", 65)] + COLS[:1], 2, [("ne", X, Y)])

    def begin(nodes):
        c = good.to_c()
        arr = (wk.WkFNode * len(nodes))(*[wk.WkFNode(*t) for t in nodes])
        c.filter = ctypes.cast(arr, ctypes.POINTER(wk.WkFNode))
        c.nfilter = len(nodes)
        return wk._eng_begin(eng._h, ctypes.byref(c))

    ne, AND, NOT = (2, -1, -2), (4, 0, 0), (6, 0, 0)
    assert begin([ne]) == 0
    assert begin([ne] * 16 + [AND] * 15 + [NOT]) == 0            # 32 nodes
    assert begin([ne] * 17 + [AND] * 16) == -3                   # 33 nodes
    assert begin([(9, -1, -2)]) == -3                            # unknown op
    assert begin([(2, -1, -3)]) == -3                            # var range
    assert begin([(2, -1, 0)]) == -3
    assert begin([AND]) == -3 and begin([ne, AND]) == -3         # underflow
    assert begin([NOT]) == -3
    assert begin([ne, ne]) == -3                                 # depth 2
    assert _same(sort_rows(eng.run_query(good)),
                 sort_rows(filter_ref.expected(ctx.ora, good)))


@pytest.mark.gpu
def test_step_api(ctx, engines):
    """execute_filter runs the whole program where the caller puts it,
    sync and async; before a variable has a column it is an error."""
    eng = engines["default"]
    for name in ("i2u-n1025-w5-clauses", "c2u-n257-w2-alt", "chain-n2049"):
        plan, want = ctx.cases[name], ctx.want(name)
        for sync in (True, False):
            eng.begin_query(plan)
            eng.execute_one_pattern()
            if plan.nvars > 1:
                with pytest.raises(ValueError):
                    eng.execute_filter()
            while eng.pattern_step < len(plan.patterns):
                eng.execute_one_pattern()
            n = eng.execute_filter(sync=sync)
            if not sync:
                assert n is None
                n = eng.row_count()
            assert n == len(want), name
            assert _same(sort_rows(eng.fetch_result(plan)), want), name


@pytest.mark.gpu
@pytest.mark.parametrize("config", list(STORE_ENVS))
def test_placement_is_exact(ctx, engines, config):
    """Same rows with pushdown on and off, with and without op chains, on
    both stores, through run_query, submit and a captured graph."""
    eng = engines[config]
    for name in list(placement_cases(ctx.g)) + ["i2u-n2049-w5-clauses"]:
        plan, want = ctx.cases[name], ctx.want(name)
        for push in (1, 0):
            for chain in (1, 0):
                with env(WK_FILTER_PUSHDOWN=push, WK_CHAIN=chain):
                    got = sort_rows(eng.run_query(plan))
                    assert _same(got, want), (name, push, chain)
                    eng.submit(plan)
                    assert eng.fetch_count() == len(want), (name, push, chain)
                    gid = eng.graph_build(plan)
                    for _ in range(2):
                        assert eng.graph_run(gid) == len(want), (name, push)
                    assert _same(sort_rows(eng.fetch_result(plan)), want)


@pytest.mark.gpu
def test_fused_steps_still_fuse(ctx):
    """With a filter behind them the 5i chain step and the 5h typeof-fused
    step still run as one step each (fewer timed launches than with
    WK_CHAIN=0 / than pattern by pattern)."""
    with env(WK_KERNEL_TIMING=1):
        eng = wk.Engine(wk.Store(ctx.triples), device=0)

    def launches(plan):
        n0 = sum(v["launches"] for v in eng.kernel_stats().values())
        eng.run_query(plan)
        return sum(v["launches"] for v in eng.kernel_stats().values()) - n0

    plan = ctx.cases["chain-n2049"]
    on = launches(plan)
    with env(WK_CHAIN=0):
        off = launches(plan)
    assert on < off, (on, off)


@pytest.mark.gpu
def test_pushdown_cuts_expansion_bytes(ctx):
    """The expansion behind a filter that drops 63 rows of 64 processes
    fewer algorithmic bytes with pushdown than without."""
    eng = wk.Engine(wk.Store(ctx.triples), device=0)
    plan = ctx.cases["pre-exp-n2049"]

    def expansion_bytes():
        s0 = eng.kernel_stats()
        eng.run_query(plan)
        s1 = eng.kernel_stats()
        return sum(s1[c]["bytes"] - s0[c]["bytes"]
                   for c in ("probe", "expand"))

    eng.run_query(plan)                       # settle the counters' base
    on = expansion_bytes()
    with env(WK_FILTER_PUSHDOWN=0):
        off = expansion_bytes()
    assert 0 < on < off, (on, off)


_CAP_CHILD = """
import os, sys
os.environ['WK_MIN_CAP'] = '64'
sys.path.insert(0, %r)
import wukong_amd as wk
import tests.test_gpu_filter_expr as T
from tests.oracle_util import sort_rows
ctx = T.Ctx()
plan, want = ctx.cases['cap'], ctx.want('cap')
assert len(want) > 4 * 64
eng = wk.Engine(wk.Store(ctx.triples), device=0)
eng.submit(plan)
assert eng.fetch_count() < 0          # the expansion overflowed 64 rows
tries = 1
eng.submit(plan)
while eng.fetch_count() < 0:
    eng.submit(plan)
    tries += 1
assert tries <= 3, tries
assert T._same(sort_rows(eng.fetch_result()), want)
eng = wk.Engine(wk.Store(ctx.triples), device=0)
assert T._same(sort_rows(eng.run_query(plan)), want)
gid = eng.graph_build(plan)
for _ in range(2):
    assert eng.graph_run(gid) == len(want)
print('FILTER_CAP_OK')
"""


@pytest.mark.gpu
def test_capacity_rerun_behind_filter():
    """WK_MIN_CAP=64 in a fresh process: the expansion behind a pushed-
    down filter overflows, the engine grows and the re-run is exact."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CAP_CHILD % (root,)],
                       capture_output=True, text=True, timeout=300)
    assert "FILTER_CAP_OK" in r.stdout, r.stdout + r.stderr
