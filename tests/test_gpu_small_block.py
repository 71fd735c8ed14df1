"""The single-block stretches of a plan: the wave-scan k_scan_local /
k_scan_mid and the fused publish+begin launch of suite captures.

The scan.  k_scan_local and k_scan_mid turn per-row counts into output
positions; every consumer (k_expand_in / _big, k_fn_scatter) writes row
r's outputs at d_pre[r] + bsums[r / chunk].  Those positions are
deterministic, so an index start followed by ONE expansion leaves a
table whose row order is fixed: input-row order (the index list,
ascending), then edge order (ascending).  `fetch_raw` is compared to a
numpy reference in exactly that order, for the non-functional pipeline
through the CSR side index (k_csr_gather -> scan -> k_expand_in) and
the functional one (k_fn_gather -> scan -> k_fn_scatter), at row counts
on every side of the 256-thread block, the 1024-row tile and the
2048-block grid cap; one wrong prefix moves a row.  The previous
barrier-ladder kernels (WK_SCAN=0) must give the same bytes.

Where a filter runs in front of the expansion the filter's own
compaction order depends on atomics, so the table order is fixed only
up to a permutation of the input rows: there the check is that every
subject's outputs are one contiguous run in edge order (that is the
`nrows < G` case: 2047..2049 rows left of 2048*256+257, G = 2048,
chunks of one or two rows).

The fused pair.  A suite capture holds query i's publish back and lets
query i+1's begin do both (k_publish_begin).  The sticky-error cases of
test_graph_replay_bookkeeping.py run again through suite captures, with
the pair fused and with WK_FUSE_PAIR=0, and must behave the same.

An OverflowError from sync is the engine's error return for a discarded
replay, not a GPU fault.
"""
import numpy as np
import pytest

import wukong_amd as wk
from wukong_amd import Plan
from tests import synth_graph as sg
from tests import test_graph_replay_bookkeeping as R
from tests.oracle_util import sort_rows
from tests.synth_graph import B, IN, OUT, TYPE

P_M, P_F = 2, 3                   # non-functional / functional
P_SEL = {2047: 4, 2048: 5, 2049: 6}   # const filters keeping K big rows
N_POOL = 700
N_BIG = 2048 * 256 + 257          # second trip of the 2048-block grid
# G = n // 256 + 2 blocks, chunk = ceil(n / G) = 256 rows: 392 * 256
# overshoots 100001 by 351 rows, so the last chunk is empty
N_TRAIL = 100001
SIZES = [1, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, N_TRAIL, N_BIG]
T_EMPTY = 399                     # a type without members: 0 rows
T_OF = {n: 400 + k for k, n in enumerate(SIZES)}
# P_M degree by member index: 0, 1, 32 | 33 (the wave-per-row queue
# starts at 33), and one row of 300 edges per set (member 5)
DEG16 = [0, 1, 32, 33, 2, 0, 1, 3, 1, 0, 2, 1, 0, 1, 0, 2]
HUB_AT, HUB_DEG = 5, 300
SPARSE_FROM = 4096                # larger sets: the pattern once per 64


def degrees(n):
    i = np.arange(n)
    if n < SPARSE_FROM:
        d = np.asarray(DEG16)[i % 16]
    else:
        d = np.where(i % 64 < 16, np.asarray(DEG16)[i % 16],
                     (i % 64 == 40).astype(int))
        d[n - 1] = HUB_DEG        # a big row in the last chunk too
    if n > HUB_AT:
        d[HUB_AT] = HUB_DEG
    return d


def scan_graph():
    nxt = [B]

    def take(k):
        a = np.arange(nxt[0], nxt[0] + k, dtype=np.uint32)
        nxt[0] += k
        return a

    pool = take(N_POOL)
    c_sel = int(take(1)[0])
    trip = []

    def add(s, p, o):
        s, o = np.broadcast_arrays(np.asarray(s, np.uint32),
                                   np.asarray(o, np.uint32))
        trip.append(np.stack([s.ravel(), np.full(s.size, p, np.uint32),
                              o.ravel()], axis=1))

    add(pool, TYPE, 398)
    subjects = {}
    for n in SIZES:
        s = take(n)
        add(s, TYPE, T_OF[n])
        d = degrees(n)
        src = np.repeat(np.arange(n), d)
        within = np.arange(int(d.sum())) - np.repeat(np.cumsum(d) - d, d)
        add(s[src], P_M, pool[(src * 7 + within) % N_POOL])
        i = np.arange(n)
        add(s[i % 3 != 0], P_F, pool[i[i % 3 != 0] % N_POOL])
        subjects[n] = s
    big = subjects[N_BIG]
    for k, pid in P_SEL.items():
        add(big[(np.arange(k) * 251) % N_BIG], pid, c_sel)
    triples = np.unique(np.concatenate(trip).astype(np.uint32), axis=0)
    return triples, dict(subjects=subjects, c_sel=c_sel)


def expand_ref(triples, subj, pid):
    """(subj, neighbour) rows: subjects in the given order, each one's
    (pid, OUT) neighbours ascending."""
    t = triples[triples[:, 1] == pid]            # np.unique order: s, then o
    lo = np.searchsorted(t[:, 0], subj, "left")
    cnt = np.searchsorted(t[:, 0], subj, "right") - lo
    idx = np.repeat(lo - (np.cumsum(cnt) - cnt), cnt) + np.arange(int(cnt.sum()))
    out = np.column_stack([np.repeat(subj, cnt), t[idx, 2]]).astype(np.uint32)
    out.setflags(write=False)
    return out


class Ctx:
    def __init__(self):
        self.triples, self.meta = scan_graph()
        self._ref = {}

    def subj(self, n):
        return (np.empty(0, np.uint32) if n == 0
                else self.meta["subjects"][n])

    def ref(self, n, pid):
        if (n, pid) not in self._ref:
            self._ref[(n, pid)] = expand_ref(self.triples, self.subj(n), pid)
        return self._ref[(n, pid)]


@pytest.fixture(scope="module")
def ctx():
    return Ctx()


@pytest.fixture(scope="module")
def eng(ctx):
    return wk.Engine(wk.Store(ctx.triples), device=0)


def plan_of(n, pid):
    return Plan([(T_OF.get(n, T_EMPTY), TYPE, IN, -1), (-1, pid, OUT, -2)],
                nvars=2, required_vars=[-1, -2])


def submit_raw(eng, plan, want_rows):
    """submit + harvest, through the engine's capacity re-run."""
    for _ in range(6):
        eng.submit(plan)
        n = eng.fetch_count()
        if n >= 0:
            assert n == want_rows, (n, want_rows)
            return eng.fetch_raw()
    raise AssertionError("capacity never settled")


# ---------------------------------------------------------------------
# CPU part: the graph has the shape the GPU tests rely on
# ---------------------------------------------------------------------
def test_scan_graph_shape(ctx):
    store = wk.Store(ctx.triples)
    k, e = store.seg_stats(P_F, OUT)
    assert k == e > 0                          # functional
    k, e = store.seg_stats(P_M, OUT)
    assert 0 < k < e                           # not functional
    assert len(store.get_index(T_EMPTY, IN)) == 0
    for n in SIZES[:10]:
        s = ctx.subj(n)
        assert np.array_equal(store.get_index(T_OF[n], IN), s)   # ascending
        d = degrees(n)
        assert n < 16 or {0, 1, 32, 33, HUB_DEG} <= set(d.tolist())
        if n > HUB_AT:
            lst = store.get_triples(int(s[HUB_AT]), P_M, OUT)
            assert len(lst) == HUB_DEG
            assert np.array_equal(lst, np.sort(lst))             # ascending
        want = ctx.ref(n, P_M)
        assert len(want) == int(d.sum())
        assert len(ctx.ref(n, P_F)) == n - (n + 2) // 3
    # trailing empty chunk of the N_TRAIL start
    g = (N_TRAIL + 256) // 256 + 1
    chunk = -(-N_TRAIL // g)
    assert g * chunk - N_TRAIL > chunk
    for k, pid in P_SEL.items():
        assert store.seg_stats(pid, OUT)[1] == k


# ---------------------------------------------------------------------
# GPU part: the scan
# ---------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("pid", [P_M, P_F], ids=["csr", "fn"])
@pytest.mark.parametrize("n", [0] + SIZES)
def test_scan_positions_exact_order(ctx, eng, n, pid):
    want = ctx.ref(n, pid)
    plan = plan_of(n, pid)
    got = submit_raw(eng, plan, len(want))
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want), "row order differs from the reference"
    with sg.env(WK_SCAN=0):
        old = submit_raw(eng, plan, len(want))
    assert np.array_equal(old, got), "ladder and wave scan differ"


@pytest.mark.gpu
@pytest.mark.parametrize("k", sorted(P_SEL))
def test_scan_fewer_rows_than_blocks(ctx, eng, k):
    """k rows left of N_BIG by a const filter: the scan grid keeps its
    2048 blocks (sized by the host bound), chunks of one or two rows,
    and for k = 2047 one block without any."""
    big = ctx.subj(N_BIG)
    kept = np.sort(big[(np.arange(k) * 251) % N_BIG])
    want = expand_ref(ctx.triples, kept, P_M)
    plan = Plan([(T_OF[N_BIG], TYPE, IN, -1),
                 (-1, P_SEL[k], OUT, ctx.meta["c_sel"]),
                 (-1, P_M, OUT, -2)], nvars=2, required_vars=[-1, -2])
    for scan in (1, 0):
        with sg.env(WK_SCAN=scan):
            got = submit_raw(eng, plan, len(want))
        assert np.array_equal(sort_rows(got), sort_rows(want)), scan
        # each subject's outputs: one contiguous run, edges ascending
        starts = np.flatnonzero(np.r_[True, got[1:, 0] != got[:-1, 0]])
        assert len(np.unique(got[starts, 0])) == len(starts), scan
        same = got[1:, 0] == got[:-1, 0]
        assert np.all(got[1:, 1][same] > got[:-1, 1][same]), scan


@pytest.mark.gpu
@pytest.mark.parametrize("pid", [P_M, P_F], ids=["csr", "fn"])
def test_scan_overflow_reports_required_rows(ctx, pid):
    """A capacity the expansion overflows (the fn pipeline cannot: its
    output is no longer than its input, it must simply pass).  The scan
    total is the exact requirement, so ONE re-run settles it, with the
    ladder and with the wave scan alike."""
    n = 1025
    want = ctx.ref(n, pid)
    attempts = {}
    with sg.env(WK_MIN_CAP=1100):
        for scan in (0, 1):
            with sg.env(WK_SCAN=scan):
                e = wk.Engine(wk.Store(ctx.triples), device=0)
                seen = []
                for _ in range(4):
                    e.submit(plan_of(n, pid))
                    seen.append(e.fetch_count())
                    if seen[-1] >= 0:
                        break
                got = e.fetch_raw()
            attempts[scan] = seen
            assert np.array_equal(got, want), scan
    print("attempts", attempts)
    assert attempts[1] == attempts[0]
    assert attempts[1] == ([-1, len(want)] if len(want) > 1100
                           else [len(want)])


# ---------------------------------------------------------------------
# GPU part: publish + begin as one launch in suite captures
# ---------------------------------------------------------------------
FUSE = [1, 0]


@pytest.fixture(scope="module")
def cctx():
    return R.ChainCtx()


@pytest.fixture(scope="module")
def chain_engines(cctx):
    return R._engines(cctx.triples)


def _suite_last(eng, plans, reps=2):
    """Replay a suite `reps` times; (discarded?, table of the last query)."""
    gid = eng.graph_build_suite(plans)
    bad = False
    for _ in range(reps):
        eng.graph_launch(gid)
        try:
            eng.sync()
        except OverflowError:
            bad = True
    return bad, eng.fetch_raw()


@pytest.mark.gpu
@pytest.mark.parametrize("fuse", FUSE)
def test_suite_of_view_starts(ctx, eng, cctx, chain_engines, fuse):
    """Every query of a suite of view-start plans last in turn: its table
    is the reference's; no replay is discarded."""
    with sg.env(WK_FUSE_PAIR=fuse):
        cases = [(257, P_M), (1025, P_F), (0, P_M), (2049, P_M)]
        for rot in range(len(cases)):
            order = cases[rot:] + cases[:rot]
            bad, raw = _suite_last(eng, [plan_of(n, p) for n, p in order])
            assert not bad, order
            want = ctx.ref(*order[-1])
            assert raw.shape == want.shape, (order, raw.shape, want.shape)
            assert np.array_equal(raw, want), order
        # the multi-step chain plans (optimistic kernels, big-row queue)
        ce = chain_engines["default"]
        c0 = cctx.meta["c0"]
        plans = [R.chain_plan("none", n, c0) for n in R.ROWS]
        for rot in range(3):
            order = plans[rot:] + plans[:rot]
            bad, raw = _suite_last(ce, order)
            assert not bad, rot
            n_last = R.ROWS[(rot + 2) % 3]
            want = cctx.want(("none", n_last), order[-1])
            assert np.array_equal(sort_rows(raw), want), rot


@pytest.mark.gpu
@pytest.mark.parametrize("store", R.STORES)
@pytest.mark.parametrize("where", ["first", "last"])
def test_suite_miss_survives(cctx, chain_engines, store, where):
    """A guard miss of the FIRST or MIDDLE query of a suite is published
    by the fused launch before the next begin clears the words: the pass
    is discarded exactly when the unfused suite's is, and with type
    bitmaps (no miss possible) never."""
    ce = chain_engines[store]
    c0 = cctx.meta["c0"]
    miss = R.chain_plan(where, 1024, c0)
    clean = R.chain_plan("none", 1025, c0)
    w_clean = cctx.want(("none", 1025), clean)
    for order in ([miss, clean, clean], [clean, miss, clean]):
        seen = {}
        for fuse in FUSE:
            with sg.env(WK_FUSE_PAIR=fuse):
                bad, raw = _suite_last(ce, order)
            seen[fuse] = bad
            if not bad:
                assert np.array_equal(sort_rows(raw), w_clean), (store, fuse)
        print(store, where, "discarded", seen)
        assert seen[1] == seen[0], (store, where, seen)
        if store == "default":
            assert not seen[1]
    # the plain path after the suites
    R._check_run_query(ce, miss, cctx.want((where, 1024), miss), (store, where))


@pytest.mark.gpu
@pytest.mark.parametrize("fuse", FUSE)
def test_suite_flag_does_not_leak(cctx, chain_engines, fuse):
    """Suites built under WK_FORCE_EMPTY_HINT=0 raise S_ERR at every
    publish (pattern 0 never leaves an empty table here), the fused ones
    included: the pass is discarded.  The same plans captured without the
    knob and replayed right after, so that their first begin follows a
    flagged publish, are exact; in one sync window with a flagged pass
    the sticky flag still reports it."""
    ce = chain_engines["default"]
    c0 = cctx.meta["c0"]
    flagged = R.chain_plan("none", 1023, c0)
    clean = R.chain_plan("none", 1025, c0)
    w_clean = cctx.want(("none", 1025), clean)
    with sg.env(WK_FUSE_PAIR=fuse):
        with sg.env(WK_FORCE_EMPTY_HINT=0):
            bad_mid = ce.graph_build_suite([clean, flagged, clean])
            bad_first = ce.graph_build_suite([flagged, clean])
        good = ce.graph_build_suite([clean, flagged, clean])
        for gid in (bad_mid, bad_first):
            ce.graph_launch(gid)
            with pytest.raises(OverflowError):
                ce.sync()
            # the next pass begins clean and is exact
            ce.graph_launch(good)
            ce.sync()
            raw = ce.fetch_raw()
            assert np.array_equal(sort_rows(raw), w_clean)
            # both in one window: the sticky flag still reports the bad one
            ce.graph_launch(gid)
            ce.graph_launch(good)
            with pytest.raises(OverflowError):
                ce.sync()
            ce.graph_launch(good)
            ce.sync()
        R._check_run_query(ce, flagged, cctx.want(("none", 1023), flagged),
                           ("after flagged suites", fuse))
