"""Device final ops (DISTINCT, OFFSET, LIMIT, projection).

The contract is the host path's output bit for bit, ROW ORDER INCLUDED:
full-row unsigned lexicographic sort, drop rows equal to their sorted
predecessor on the required columns, slice, project.  `final_ref` restates
that in numpy; its authority comes from two checks made on every case — it
equals the host arm (WK_DEV_FINAL=0, same process, read per call) and, on
the whole-query cases, OracleCtx.run_query.  All comparisons are
np.array_equal on the unsorted output.

Tables are injected with load_rbuf so the shapes are exact.  The final-op
grid gives every block a contiguous range that is a multiple of the 256-row
tile, so at these sizes one block owns one tile: 255/256/257 sit on the
tile edge and 769 is three tiles plus one row.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import wukong_amd as wk
from wukong_amd import Plan
from wukong_amd import queries as Q
from tests.oracle_util import sort_rows
from tests.synth_graph import env

BLANK = 0xFFFFFFFF
TILE = 256
ROWS = [0, 1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 1]
COLS = [1, 2, 3, 8]
X, Y, Z = Q.X, Q.Y, Q.Z


# ---------------------------------------------------------------------
# numpy restatement of finalize_result
# ---------------------------------------------------------------------
def final_ref(table, v2c, req, distinct=False, limit=-1, offset=0):
    t = np.asarray(table, dtype=np.uint32)
    cols = [v2c[-(v + 1)] for v in req]
    if distinct and len(t):
        t = t[np.lexsort(t.T[::-1])]          # stable, column 0 major
        keep = np.ones(len(t), dtype=bool)
        have = [c for c in cols if c >= 0]
        if have:
            keep[1:] = (t[1:][:, have] != t[:-1][:, have]).any(axis=1)
        else:
            keep[1:] = False
        t = t[keep]
    if offset > 0:
        t = t[offset:]
    if limit >= 0:
        t = t[:limit]
    out = np.full((len(t), len(req)), BLANK, dtype=np.uint32)
    for j, c in enumerate(cols):
        if c >= 0:
            out[:, j] = t[:, c]
    return out


def _same(got, want):
    return got.shape == want.shape and np.array_equal(got, want)


def make_table(kind, n, c, rng):
    """(n, c) uint32 tables that put the sort on its edges."""
    t = np.full((n, c), 0x00ABCDEF, dtype=np.uint32)
    r = np.arange(n, dtype=np.uint64)
    if kind == "same":
        pass
    elif kind == "distinct":      # every row unique, in shuffled order
        t[:] = rng.integers(0, 1 << 32, size=(n, c), dtype=np.uint64)
        t[:, 0] = (rng.permutation(n).astype(np.uint64) * 2654435761) % (1 << 32)
    elif kind == "top":           # keys differ in the top byte only
        t[:, 0] = ((rng.integers(0, 256, n, dtype=np.uint64) << 24) | 0x123456)
    elif kind == "low":           # ... in the low byte only
        t[:, 0] = 0x12345600 | rng.integers(0, 256, n, dtype=np.uint64)
    elif kind == "last":          # ... in the last column only
        t[:, c - 1] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    elif kind == "unsigned":      # >= 2^31 next to small ones, BLANK_ID
        pool = np.array([0, 1, 5, 0x7FFFFFFF, 0x80000000, 0x80000007,
                         0xFFFFFFFE, BLANK], dtype=np.uint32)
        t[:] = pool[rng.integers(0, len(pool), size=(n, c))]
    elif kind == "dups":          # few values: many duplicate rows
        t[:] = rng.integers(0, 3, size=(n, c), dtype=np.uint64)
    elif kind == "stab":          # column 0 constant, column 1 decides
        t[:, min(1, c - 1)] = (r * 7919) % 251
    else:
        raise KeyError(kind)
    return t


KINDS = ["same", "distinct", "top", "low", "last", "unsigned", "dups", "stab"]


def req_sets(c):
    """name -> (nvars, v2c, required vars) for a table of c columns."""
    ident = list(range(c))
    out = {"all": (c, ident, [-(i + 1) for i in range(c)])}
    if c >= 2:
        out["single"] = (c, ident, [-c])
        out["repeat"] = (c, ident, [-1, -1, -c])
    if c >= 3:
        out["pair"] = (c, ident, [-1, -3])           # not a prefix
    if c < 8:
        out["nocol"] = (c + 1, ident + [-1], [-1, -(c + 1)])
    return out


def _plan(nvars, req, **kw):
    # the pattern list is irrelevant once a table is loaded
    return Plan([(Q.COURSE, Q.TYPE_ID, wk.DIR_IN, -1)], nvars, req, **kw)


def run_final(eng, table, v2c, plan):
    eng.begin_query(plan)
    eng.load_rbuf(table, v2c, step=len(plan.patterns))
    return eng.fetch_result(plan)


def check(eng, table, nvars, v2c, req, **kw):
    plan = _plan(nvars, req, **kw)
    want = final_ref(table, v2c, req, **kw)
    got = run_final(eng, table, v2c, plan)
    with env(WK_DEV_FINAL=0):
        host = run_final(eng, table, v2c, plan)
    tag = (table.shape, req, kw)
    assert _same(host, want), ("host != numpy", tag)
    assert _same(got, want), ("device != numpy", tag, got[:8], want[:8])
    return want


# ---------------------------------------------------------------------
# CPU part
# ---------------------------------------------------------------------
def test_surface_exists():
    """The new C symbols are exported and wrapped."""
    for name in ("wk_engine_final_count", "wk_engine_final_passes"):
        assert hasattr(wk._lib, name), name
    assert callable(getattr(wk.Engine, "final_count", None))


def test_reference_keeps_non_adjacent_duplicates():
    """Rows equal on a non-prefix pair of required columns that are not
    adjacent after the full-row sort both survive."""
    t = np.array([[7, 1, 4], [7, 2, 5], [7, 3, 4], [7, 3, 4]], dtype=np.uint32)
    out = final_ref(t, [0, 1, 2], [-1, -3], distinct=True)
    assert out.tolist() == [[7, 4], [7, 5], [7, 4]]
    # unsigned order, BLANK_ID last
    t = np.array([[BLANK], [0x80000000], [1]], dtype=np.uint32)
    assert final_ref(t, [0], [-1], distinct=True)[:, 0].tolist() == \
        [1, 0x80000000, BLANK]


# ---------------------------------------------------------------------
# GPU part
# ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng(store4):
    return wk.Engine(store4, device=0)


@pytest.fixture(autouse=True)
def _always_device():
    """Small non-captured fetches default to the host final ops
    (WK_FINAL_HOST_ROWS); these tests are about the device pass."""
    with env(WK_FINAL_HOST_ROWS=0):
        yield


@pytest.mark.gpu
@pytest.mark.parametrize("c", COLS)
def test_distinct_sweep(eng, c):
    """Row counts x value kinds x required-var sets, DISTINCT."""
    rng = np.random.default_rng(1000 + c)
    survivors = False
    for n in ROWS:
        for kind in KINDS:
            t = make_table(kind, n, c, rng)
            for name, (nvars, v2c, req) in req_sets(c).items():
                if name != "all" and kind not in ("dups", "unsigned", "distinct"):
                    continue
                want = check(eng, t, nvars, v2c, req, distinct=True)
                if name == "pair" and kind == "dups" and n >= 63:
                    # the non-prefix case: a required-column duplicate that
                    # was not adjacent survives in the expected output
                    survivors |= len(np.unique(want, axis=0)) < len(want)
                if name == "nocol" and n:
                    assert (want[:, 1] == BLANK).all()
    assert survivors or c < 3


@pytest.mark.gpu
def test_stability_and_pass_skipping(eng):
    """Column 0 constant: the order is column 1's alone; the constant
    digits are skipped on the device, and skipping changes nothing."""
    n = 3 * TILE + 1
    t = np.full((n, 2), 0x00ABCDEF, dtype=np.uint32)
    t[:, 1] = (np.arange(n, dtype=np.uint64) * 7919) % 251
    want = check(eng, t, 2, [0, 1], [-1, -2], distinct=True)
    assert len(want) == 251 and (np.diff(want[:, 1].astype(np.int64)) > 0).all()
    run_final(eng, t, [0, 1], _plan(2, [-1, -2], distinct=True))
    assert eng.final_passes() == (1, 8)      # values < 256 in one column
    t[0, 0] = BLANK                          # every digit of column 0 varies
    check(eng, t, 2, [0, 1], [-1, -2], distinct=True)
    run_final(eng, t, [0, 1], _plan(2, [-1, -2], distinct=True))
    assert eng.final_passes() == (5, 8)


@pytest.mark.gpu
@pytest.mark.parametrize("distinct", [False, True])
def test_offset_limit(eng, distinct):
    rng = np.random.default_rng(7)
    n = 3 * TILE + 1
    for kind in ("distinct", "dups"):
        t = make_table(kind, n, 2, rng)
        m = len(final_ref(t, [0, 1], [-1, -2], distinct=distinct))
        if distinct and kind == "dups":
            assert m == 9
        cuts = sorted({0, 3, TILE - 6, m, m + 5, n, n + 5})
        for offset in cuts:
            check(eng, t, 2, [0, 1], [-2, -1], distinct=distinct, offset=offset)
        for limit in cuts:
            check(eng, t, 2, [0, 1], [-2, -1], distinct=distinct, limit=limit)
        # offset and limit straddling a block boundary
        for offset, limit in ((TILE - 6, 20), (TILE - 1, 2), (2 * TILE - 3, TILE + 9),
                              (m, 0), (m - 1 if m else 0, 5)):
            check(eng, t, 2, [0, 1], [-2, -1], distinct=distinct,
                  offset=offset, limit=limit)


@pytest.mark.gpu
def test_final_count_and_fetch_raw(eng):
    rng = np.random.default_rng(3)
    t = make_table("dups", 3 * TILE + 1, 3, rng)
    v2c = [0, 1, 2]
    plan = _plan(3, [-3, -1], distinct=True, offset=2)
    eng.begin_query(plan)
    eng.load_rbuf(t, v2c, step=1)
    with pytest.raises(RuntimeError):
        eng.final_count()                    # no final pass yet
    got = eng.fetch_result(plan)
    assert _same(got, final_ref(t, v2c, [-3, -1], distinct=True, offset=2))
    assert eng.final_count() == len(got)
    # the pre-final table is still the current one
    assert _same(eng.fetch_raw(), t)
    assert _same(eng.fetch_result(plan), got)
    assert eng.final_count() == len(got)
    eng.load_rbuf(t, v2c, step=1)            # a new table drops the mark
    with pytest.raises(RuntimeError):
        eng.final_count()
    # below the row cutoff a non-captured fetch keeps the host path: same
    # rows, and the count is there too
    with env(WK_FINAL_HOST_ROWS=8192):
        assert _same(run_final(eng, t, v2c, plan), got)
        assert eng.final_count() == len(got)
        with pytest.raises(RuntimeError):
            eng.final_passes()               # no device pass ran
    # blind counts stay pre-final
    assert eng.run_query_count(Plan(Q.Q2.patterns, 2, [X], distinct=True)) == \
        eng.run_query_count(Q.Q2)


def _q2d():
    return Plan(Q.Q2.patterns, 2, [X], distinct=True)


def _q7d():
    return Plan(Q.Q7.patterns, 3, [X, Y, Z], distinct=True, offset=3, limit=40)


def _pairs():
    return Plan([(Q.DEPT0_UNIV0, Q.MEMBEROF, wk.DIR_IN, X),
                 (X, Q.ADVISOR, wk.DIR_OUT, Y),
                 (Y, Q.ADVISOR, wk.DIR_IN, Z)], 3, [X, Z],
                distinct=True, limit=40, offset=3, filters=[("ne", X, Z)])


@pytest.mark.gpu
def test_whole_queries(eng, oracle4):
    for plan in (_q2d(), _q7d()):
        want = oracle4.run_query(plan)
        assert len(want)
        got = eng.run_query(plan)
        assert _same(got, want), (got.shape, want.shape)
        assert eng.final_count() == len(want)
        with env(WK_DEV_FINAL=0):
            assert _same(eng.run_query(plan), want)
    # FILTER + DISTINCT/LIMIT/OFFSET: the oracle has no FILTER — host arm
    plan = _pairs()
    with env(WK_DEV_FINAL=0):
        want = eng.run_query(plan)
    assert len(want) > 0
    assert _same(eng.run_query(plan), want)


@pytest.mark.gpu
def test_zero_copy_view(eng, oracle4):
    """The current table is the store's own edge list (index start, one
    pattern): the final pass reads it in place and never writes it."""
    pats = [(Q.COURSE, Q.TYPE_ID, wk.DIR_IN, X)]
    plan = Plan(pats, 1, [X], distinct=True)
    want = oracle4.run_query(plan)
    assert len(want) > TILE
    assert _same(eng.run_query(plan), want)
    bare = Plan(pats, 1, [X])
    assert _same(sort_rows(eng.run_query(bare)), sort_rows(oracle4.run_query(bare)))
    # step API: fetch_raw after the device fetch is still the edge list
    eng.begin_query(plan)
    eng.execute_one_pattern()
    assert _same(eng.fetch_result(plan), want)
    assert _same(sort_rows(eng.fetch_raw()), sort_rows(oracle4.run_query(bare)))


@pytest.mark.gpu
def test_graph_replay(eng):
    q2w = Plan(Q.Q2.patterns, 2, [X, Y], limit=100, offset=100)
    for plan in (_q2d(), q2w):
        want = eng.run_query(plan)
        blind = eng.run_query_count(plan)
        assert 0 < len(want) <= blind
        gid = eng.graph_build(plan)          # rc = -3 before this feature
        for _ in range(3):
            assert eng.graph_run(gid) == blind
            assert eng.final_count() == len(want)
        assert _same(eng.fetch_result(plan), want)
        assert eng.final_count() == len(want)
        # another plan's fetch recomputes instead of reusing the table
        other = Plan(plan.patterns, 2, [X], distinct=True, limit=5)
        assert eng.graph_run(gid) == blind
        assert _same(eng.fetch_result(other), eng.run_query(other))
    # a replay of a graph without final ops drops the mark
    g1 = eng.graph_build(Q.Q1)
    eng.graph_run(g1)
    with pytest.raises(RuntimeError):
        eng.final_count()


@pytest.mark.gpu
def test_graph_suite_and_knob(eng):
    q7l = Plan(Q.Q7.patterns, 3, [X, Y, Z], limit=40, offset=3)
    plans = [Q.Q1, _q2d(), q7l]
    gid = eng.graph_build_suite(plans)
    eng.graph_launch(gid)
    eng.sync()
    assert _same(eng.run_query(_q2d()), final_ref(
        eng.run_query(Q.Q2), [0, 1], [X], distinct=True))
    with env(WK_DEV_FINAL=0):
        for plan in (_q2d(), q7l):
            with pytest.raises(RuntimeError, match="rc=-3"):
                eng.graph_build(plan)
        with pytest.raises(RuntimeError, match="rc=-3"):
            eng.graph_build_suite(plans)


_CAP_CHILD = """
import os, sys
os.environ['WK_MIN_CAP'] = '64'
os.environ['WK_FINAL_HOST_ROWS'] = '0'
sys.path.insert(0, %r)
import numpy as np
import wukong_amd as wk
from wukong_amd import Plan, queries as Q
from tests.oracle_util import OracleCtx
tri = wk.lubm_gen(2, seed=42)
eng = wk.Engine(wk.Store(tri), device=0)
ora = OracleCtx(tri)
for plan in (Plan(Q.Q2.patterns, 2, [Q.X], distinct=True),
             Plan(Q.Q7.patterns, 3, [Q.X, Q.Y, Q.Z], distinct=True,
                  offset=3, limit=40)):
    want = ora.run_query(plan)
    assert len(want) > 0
    eng = wk.Engine(wk.Store(tri), device=0)      # tiny caps again
    got = eng.run_query(plan)                     # overflows, grows, re-runs
    assert got.shape == want.shape and np.array_equal(got, want)
    assert eng.final_count() == len(want)
assert eng.run_query_count(Q.Q2) > 4 * 64
print('FINAL_CAP_OK')
"""


@pytest.mark.gpu
def test_capacity_rerun():
    """WK_MIN_CAP=64 in a fresh process: the table of a DISTINCT query
    outgrows the caps, the engine grows and the re-run is exact."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CAP_CHILD % (root,)],
                       capture_output=True, text=True, timeout=300)
    assert "FINAL_CAP_OK" in r.stdout, r.stdout + r.stderr
