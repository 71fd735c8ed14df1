"""Batched (op-major) chain evaluation in the chain-fused CSR expansion
(DESIGN.md §3 5i): the count pass walks CHAIN_RPT = 2 rows side by side
(rows r and r + ceil(n / 2) of an n-row table below the grid size),
CHAIN_EK edges of each per round, with clamped always-valid loads for
inactive or failed candidates, and leaves a 32-bit pass mask per row; the
writer takes the passing edges of a <= 32-edge row from that mask and
repeats only the FN_APPEND lookups.

The graph below is built for the shapes that code can get wrong: an edge
ladder around the group size K = 4, the 32-edge mask and the 64-edge wave
chunks, rows whose ONLY passing edge sits at position 0, at position 31,
or in the last partial group, chains that pass everything and nothing,
appended values that feed a later FN_EQ and TYPE, absent keys in the
middle of a group, a one-key map, a map keyed once per 64 vids, lookups
with type ids (far below every span) and with the largest vid of the
graph (last page / last bitmap word).  Spans are store-wide, so a vid
above them cannot occur in a table; vid 0 is not a vertex.  Every
comparison is exact: sorted row sets against the oracle and against the
same engine with WK_CHAIN=0.  The `rp-*` plans are runs of per-row
patterns with no expansion in front (a stand-alone pass over the start
table, a zero-copy i2u or c2u view): keep rates none / one row / one row
per 64 / all, and a FILTER conjunct bound inside the run.  Such a run
keeps at most its input rows, and the start step has already sized the
capacity for those, so it cannot overflow; the 64-row capacity case runs
it behind an overflowing expansion instead.

CPU part (unmarked): oracle == brute for every plan of the file, and the
graph has the properties the GPU cases rely on.
"""
import numpy as np
import pytest

import wukong_amd as wk
from wukong_amd import Plan
from tests import filter_ref
from tests.oracle_util import OracleCtx, sort_rows
from tests.synth_graph import B, IN, OUT, TYPE, env

K = 4                               # CHAIN_EK: edges per evaluation round
NA = 1031                           # prime: no multiple of K or of the row pairs
ROWS = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, NA]
LAD = [0, 1, K - 1, K, K + 1, 2 * K + 1, 31, 32, 33, 64, 65]
HUB, HUB2, HUB_DEG = 12, 700, 300   # one hub in each half of the row pairs
NCP = 400                           # course pool
STRIDE = 37

P_E, P_OWN, P_LBL, P_LBL2, P_BACK, P_BACK2, P_ONE, P_W, P_G, P_G2 = range(2, 12)
P_A1, P_AW = 12, 13
T_CALL, T_NONE, T_LALL, T_L1, T_D = range(20, 25)
T_R0 = 40                           # T_R0 + i: first ROWS[i] subjects

STORE_ENVS = {
    "default": {},
    "hash": dict(WK_FN=0, WK_CSR=0, WK_TBM=0),
    "notbm": dict(WK_TBM=0),
}


def r_type(n):
    return T_R0 + ROWS.index(n)


def deg_of(q):
    return HUB_DEG if q in (HUB, HUB2) else LAD[q % len(LAD)]


def start_of(q):
    return (q * STRIDE) % (NCP - deg_of(q) + 1)


def want_pos(q):
    """The one position row q is meant to pass P_OWN at (None: no wish)."""
    d = deg_of(q)
    if d == 0 or q in (HUB, HUB2):
        return None
    if d == 32:
        return 0 if (q // len(LAD)) % 2 == 0 else 31
    return d - 1 if d >= K else 0   # the last (partial) group, or edge 0


def batch_graph():
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

    A, C, L, D = take(NA), take(NCP), take(NCP), take(16)
    Z = take(1)                     # default owner: never a subject
    VMAX = take(1)                  # the largest vid: an edge target only
    m = np.arange(NCP)
    # expansion predicate: row q -> C[start .. start + deg), contiguous, so
    # the position of an edge in the (sorted) list is its offset
    for q in range(NA):
        d = deg_of(q)
        if d:
            add(A[q], P_E, C[start_of(q) + np.arange(d)])
    add(A[5], P_E, VMAX)            # 9 + 1 edges, the last one is VMAX
    # owner of a course (functional): absent when m % 3 == 0, else Z, then
    # the hub's own edges and the wished (row, position) pairs, first come
    # first served
    owner = {int(i): int(Z[0]) for i in m if i % 3}
    taken = set()
    for hq in (HUB, HUB2):          # the hubs' own edges
        for p in (0, 31, 32, 63, 64, 65, 127, 128, 299):
            ci = start_of(hq) + p
            if ci not in taken:
                taken.add(ci)
                owner[ci] = int(A[hq])
    for q in range(NA):
        p = want_pos(q)
        if p is None:
            continue
        ci = start_of(q) + p
        if ci not in taken:
            taken.add(ci)
            owner[ci] = int(A[q])
    ks = np.array(sorted(owner))
    add(C[ks], P_OWN, np.array([owner[int(i)] for i in ks], np.uint32))
    add(C, TYPE, T_CALL)
    add(A[0], TYPE, T_NONE)         # a bitmap no course is in
    add(C, P_LBL, L[m])                               # every course
    add(C[m % 5 != 0], P_LBL2, L[m[m % 5 != 0]])      # key absent if m%5==0
    add(L, TYPE, T_LALL)
    add(L[m % 2 == 0], TYPE, T_L1)
    add(L, P_BACK2, C[m])                             # back2[label] == course
    add(L, P_BACK, C[np.where(m % 3 != 0, m, (m + 1) % NCP)])
    add(C[17], P_ONE, L[0])                           # a one-key map
    w = C % 64 == 0
    add(C[w], P_W, L[m[w]])                           # one key per 64 vids
    q = np.arange(NA)
    add(A, P_G, D[q % 16])
    add(A, P_G2, D[(q * 3) % 16])
    add(D, TYPE, T_D)
    add(A[3], P_A1, D[0])                             # one subject only
    add(A[q % 64 == 0], P_AW, D[1])                   # one subject per 64
    for n in ROWS:
        if n:
            add(A[:n], TYPE, r_type(n))
    meta = dict(A=A, C=C, L=L, D=D, VMAX=int(VMAX[0]))
    return np.concatenate(trip).astype(np.uint32), meta


def _plan(pats, nvars):
    return Plan(pats, nvars=nvars,
                required_vars=[-(v + 1) for v in range(nvars)])


def plans(t):
    a, b, c, d, g, h = -1, -2, -3, -4, -5, -6
    s0 = (t, TYPE, IN, a)
    ex = (a, P_E, OUT, b)
    ops = [(b, TYPE, OUT, T_CALL), (b, P_LBL, OUT, c), (c, TYPE, OUT, T_LALL),
           (c, P_BACK2, OUT, b), (b, P_LBL2, OUT, d), (d, TYPE, OUT, T_L1),
           (d, P_BACK, OUT, b), (b, TYPE, OUT, T_CALL)]
    out = {
        # chain length 1 (FN_EQ): one passing edge per row, by position
        "own": _plan([s0, ex, (b, P_OWN, OUT, a)], 2),
        "all": _plan([s0, ex, ops[0], ops[1]], 3),
        "none": _plan([s0, ex, (b, TYPE, OUT, T_NONE), ops[1]], 3),
        # the appended value feeds a TYPE and an FN_EQ; absent append keys
        "feed": _plan([s0, ex, (b, P_LBL2, OUT, c), (c, TYPE, OUT, T_L1),
                       (c, P_BACK, OUT, b)], 3),
        "onekey": _plan([s0, ex, (b, P_ONE, OUT, c), ops[0]], 3),
        "per64": _plan([s0, ex, (b, P_W, OUT, c), ops[0]], 3),
        # type ids as keys: below every map and bitmap span
        "typeids-fn": _plan([s0, (a, TYPE, OUT, b), ops[1], ops[2]], 3),
        "typeids-type": _plan([s0, (a, TYPE, OUT, b), (a, P_G, OUT, c),
                               (b, TYPE, OUT, T_CALL)], 3),
        # input widths 2 and 3
        "w2": _plan([s0, (a, P_G, OUT, c), (a, P_E, OUT, b),
                     (b, P_OWN, OUT, a), (b, P_LBL, OUT, d)], 4),
        "w3": _plan([s0, (a, P_G, OUT, c), (a, P_G2, OUT, d),
                     (a, P_E, OUT, b), (b, P_OWN, OUT, a)], 4),
    }
    for k in range(2, 9):
        nv = 2 + sum(1 for o in ops[:k] if o[3] in (c, d) and o[0] == b)
        out["len%d" % k] = _plan([s0, ex] + ops[:k], nv)
    # runs of per-row patterns right behind the (zero-copy) start table
    d0 = B + NA + 2 * NCP           # vid of D[0]
    isd = (b, TYPE, OUT, T_D)
    out.update({
        "rp-all": _plan([s0, (a, P_G, OUT, b), isd], 2),
        "rp-none": _plan([s0, (a, P_G, OUT, b), (b, TYPE, OUT, T_NONE)], 2),
        "rp-one": _plan([s0, (a, P_A1, OUT, b), isd], 2),
        "rp-wave": _plan([s0, (a, P_AW, OUT, b), isd], 2),
        "rp-len4": _plan([s0, (a, P_G, OUT, b), isd, (a, P_G2, OUT, c),
                          (a, P_AW, OUT, d)], 4),
        # c2u start: the subjects of department 0, narrowed to this set
        "rp-c2u": _plan([(d0, P_G, IN, a), (a, P_G2, OUT, b), isd,
                         (a, TYPE, OUT, t)], 2),
        # FILTER conjunct whose last variable is bound inside the run
        "rp-filter": Plan([s0, (a, P_G, OUT, b), isd, (a, P_G2, OUT, c)],
                          nvars=3, required_vars=[-1, -2, -3],
                          filters=[("ne", b, c)]),
        # the run behind an expansion that overflows a small capacity
        "rp-cap": _plan([s0, (a, P_G, OUT, c), (c, TYPE, OUT, T_D), ex], 3),
    })
    return out


def all_cases():
    out = []
    for n in ROWS:
        for k, p in plans(r_type(n)).items():
            out.append(("%s-n%d" % (k, n), p))
    return out


def _same(got, want):
    if len(got) == 0 or len(want) == 0:
        return len(got) == len(want)
    return got.shape == want.shape and np.array_equal(got, want)


class Ctx:
    def __init__(self):
        self.triples, self.meta = batch_graph()
        self.ora = OracleCtx(self.triples)
        self.cases = all_cases()
        self.by_name = dict(self.cases)
        self._want = {}

    def want(self, name):
        if name not in self._want:
            r = sort_rows(filter_ref.expected(self.ora, self.by_name[name]))
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
        bare = filter_ref.unfiltered(plan)      # brute knows no FILTER
        a = sort_rows(ctx.ora.run_query(bare))
        b = sort_rows(ctx.ora.brute_query(bare))
        assert _same(a, b), name


def test_graph_properties(ctx):
    store = wk.Store(ctx.triples)
    assert store.check() == 0
    A, C = ctx.meta["A"], ctx.meta["C"]
    for p in (P_OWN, P_LBL, P_LBL2, P_BACK, P_BACK2, P_ONE, P_W, P_G, P_G2):
        k, e = store.seg_stats(p, OUT)
        assert k == e > 0, p                      # functional
    assert store.seg_stats(P_ONE, OUT)[0] == 1
    wkeys = store.seg_stats(P_W, OUT)[0]
    assert wkeys == int((C % 64 == 0).sum()) >= NCP // 64
    k, e = store.seg_stats(P_E, OUT)
    assert 0 < k < e and e // k <= 32             # chain-fused gate
    # the edge ladder, as stored
    degs = {len(store.get_triples(int(A[q]), P_E, OUT)) for q in range(NA)}
    assert degs >= {1, K - 1, K, K + 1, 31, 32, 33, 64, 65, HUB_DEG}
    assert len(store.get_triples(int(A[0]), P_E, OUT)) == 0
    lst5 = store.get_triples(int(A[5]), P_E, OUT)
    assert len(lst5) == 2 * K + 2 and int(lst5[-1]) == ctx.meta["VMAX"]
    assert ctx.meta["VMAX"] == int(ctx.triples[:, [0, 2]].max())
    # passing positions of the FN_EQ chain, per row, from the oracle
    own = ctx.want("own-n%d" % NA)
    pos = {}
    for x, y in own.tolist():
        q = x - int(A[0])
        pos.setdefault(q, []).append(y - int(C[0]) - start_of(q))
    only = lambda d, p: any(deg_of(q) == d and v == [p] for q, v in pos.items())
    assert only(32, 0) and only(32, 31)           # mask bit 0 / bit 31 alone
    assert only(33, 32) and only(65, 64) and only(64, 63)
    assert only(2 * K + 1, 2 * K) and only(K + 1, K)   # last partial group
    assert only(K, K - 1) and only(K - 1, 0) and only(1, 0)
    for hq in (HUB, HUB2):
        assert len(pos[hq]) >= 4 and len({p // 64 for p in pos[hq]}) >= 3
    # the count pass pairs rows r and r + ceil(n / 2): the degree pairs
    # that share a thread, per row count
    def pairs(n):
        h = (n + 1) // 2
        return {(deg_of(r), deg_of(r + h)) for r in range(h) if r + h < n}
    assert pairs(NA) >= {(33, 32), (64, 33), (0, 65), (1, 0), (32, 31),
                         (HUB_DEG, 0), (33, HUB_DEG)}
    assert pairs(1025) >= {(0, 32), (1, 33), (K - 1, 64), (K, 65)}
    assert pairs(1023) >= {(0, 31), (1, 32), (K - 1, 33), (K + 1, 65)}
    assert pairs(65) and pairs(257) and not pairs(1)
    n = NA
    w = lambda k_: len(ctx.want("%s-n%d" % (k_, n)))
    assert w("all") == e - 1                      # all but the VMAX edge
    assert w("none") == 0 and w("typeids-fn") == 0 and w("typeids-type") == 0
    assert w("onekey") >= 1 and w("per64") >= 1
    assert 0 < w("feed") < w("all")
    for k_ in range(2, 9):
        assert w("len%d" % k_) > 0, k_
    assert w("len8") < w("len4") == w("all")
    assert w("w2") > 0 and w("w3") == w("own")
    # a one-row table keeps nothing (row 0 has no edge), an empty one too
    assert len(ctx.want("own-n1")) == 0 and len(ctx.want("own-n63")) > 1
    assert len(ctx.want("all-n0")) == 0
    # the stand-alone runs: all / none / one row / one row per 64
    assert w("rp-all") == n and w("rp-none") == 0 and w("rp-one") == 1
    assert w("rp-wave") == (n + 63) // 64 == w("rp-len4")
    assert w("rp-c2u") == (n + 15) // 16
    assert 0 < w("rp-filter") < n
    assert len(ctx.want("rp-one-n1")) == 0 and len(ctx.want("rp-all-n1")) == 1
    assert len(ctx.want("rp-cap-n65")) > 20 * 64


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


def _check(eng, ctx, name):
    plan, want = ctx.by_name[name], ctx.want(name)
    for path in ("run_query", "submit"):
        got = _rows(eng, plan, path)
        assert _same(got, want), (name, path, got.shape, want.shape)
        with env(WK_CHAIN=0):
            ref = _rows(eng, plan, path)
        assert _same(ref, got), (name, path)


@pytest.mark.gpu
@pytest.mark.parametrize("config", list(STORE_ENVS))
def test_plans_exact(ctx, engines, config):
    eng = engines[config]
    for name, _ in ctx.cases:
        _check(eng, ctx, name)


@pytest.mark.gpu
def test_span_top_is_largest_vid(ctx, engines):
    """The store-wide spans start at B and end at the largest vid, so the
    VMAX edge lands on the last index of every page and bitmap array."""
    blob = wk.WkPeerBlob.from_buffer_copy(engines["default"]._store.export_blob())
    assert blob.type_base == B
    assert blob.type_base + blob.type_n - 1 == ctx.meta["VMAX"]


@pytest.mark.gpu
def test_chain_kernels_run(ctx):
    """The plans of this file do take the fused step: fewer timed launches
    than with WK_CHAIN=0.  (A two-pattern run of a functional k2u and a
    type test on its value is one timed launch either way, so the row
    pass is counted on its longer runs.)"""
    with env(WK_KERNEL_TIMING=1):
        eng = wk.Engine(wk.Store(ctx.triples), device=0)

    def launches(plan):
        n0 = sum(v["launches"] for v in eng.kernel_stats().values())
        eng.run_query(plan)
        return sum(v["launches"] for v in eng.kernel_stats().values()) - n0

    for key in ("own", "feed", "len8", "w3", "rp-len4", "rp-c2u"):
        plan = ctx.by_name["%s-n%d" % (key, NA)]
        on = launches(plan)
        with env(WK_CHAIN=0):
            off = launches(plan)
        assert on < off, (key, on, off)


@pytest.mark.gpu
def test_graph_replay(ctx, engines):
    eng = engines["default"]
    for name in [c[0] for c in ctx.cases
                 if c[0].endswith(("-n0", "-n65", "-n%d" % NA))]:
        plan, want = ctx.by_name[name], ctx.want(name)
        gid = eng.graph_build(plan)
        for _ in range(2):
            assert eng.graph_run(gid) == len(want), name
            got = sort_rows(eng.fetch_result(plan))
            assert _same(got, want), name


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["all-n63", "len4-n65", "rp-cap-n65"])
def test_capacity_rerun(ctx, engines, key):
    """A 64-row capacity overflows inside the chain step (every edge
    passes, with appended columns): the first fetch reports it, the
    writers clamp at `cap`, the engine grows and the re-run is exact."""
    gstore = engines["default"]._store
    plan, want = ctx.by_name[key], ctx.want(key)
    assert len(want) > 20 * 64
    with env(WK_MIN_CAP=64):
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
