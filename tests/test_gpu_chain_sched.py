"""Round-scheduled op chains.

chain_eval_batch walks a chain in dependency rounds of up to CHAIN_SLOTS ops
(wk_chain_sched.h): ops that do not read each other's appended column share
a round, every FN_APPEND keeps the column it has in plan order, and a wave
without a live candidate leaves the round loop.  WK_CHAIN_SCHED=0
gives one op per round in plan order (no early-out), WK_CHAIN_GRID=<n> caps
the chain kernels' grids so that one block walks several tiles of a small
table.  Every arm must give the oracle's rows, exactly, as sorted row
multisets.

The graph is test_gpu_chain_width's (2049 subjects, the P_E ladder of 0..40
edges) plus three predicates of this file: P_LD (label -> department, equal
to the subject's P_G department for even subjects), P_CA (course -> the one
subject whose FIRST P_E edge it is) and one type per start size that holds
only that start set's last subject.

CPU part (unmarked): the scheduler header, compiled into a stand-alone
program, against the schedule's properties on random chains; oracle == brute
for every plan; and the keep rates the GPU cases rely on.
"""
import os
import random
import subprocess

import numpy as np
import pytest

import wukong_amd as wk
from wukong_amd import build as wk_build
from tests.oracle_util import OracleCtx, sort_rows
from tests.synth_graph import IN, OUT, TYPE, env
from tests.test_gpu_chain_width import (
    NA, NCP, ND, ROWS, P_G, P_G2, P_H, P_E, P_CL, P_BACK, P_DH, P_EH, P_R,
    T_D, T_X, T_C1, T_HALF, T_NONE, T_L, r_type, width_graph, _plan, _same)

P_LD, P_CA = 11, 12
T_LAST0 = 60                                # T_LAST0 + i: A[ROWS[i] - 1] only
CHAIN_MAX, CHAIN_SLOTS = 8, 2
FN_APPEND, CH_TYPE, FN_EQ, CH_EQ = range(4)

ARMS = {
    "default": {},
    "sched0": dict(WK_CHAIN_SCHED=0),
    "wide": dict(WK_CHAIN_WIDTH=8),
    "grid1": dict(WK_CHAIN_GRID=1),
    "unfused": dict(WK_CHAIN=0),
}


def last_type(n):
    return T_LAST0 + ROWS.index(n)


def sched_graph():
    base, meta = width_graph()
    A, C, L, D = meta["A"], meta["C"], meta["L"], meta["D"]
    q = np.arange(NA)
    m = np.arange(NCP)
    col = lambda s, p, o: np.stack(
        [np.asarray(s, np.uint32), np.full(len(s), p, np.uint32),
         np.asarray(o, np.uint32)], axis=1)
    extra = [
        col(L, P_LD, D[np.where(q % 2 == 0, q, q + 1) % ND]),
        # subject i's k-th edge is C[(7 i + k) % 211] and 7 * 181 = 1 (211)
        col(C, P_CA, A[(m * 181) % NCP]),
    ]
    for n in ROWS:
        extra.append(col(A[n - 1:n], TYPE, [last_type(n)]))
    t = np.concatenate([base] + extra).astype(np.uint32)
    return np.unique(t, axis=0), meta


def row_plans(n, meta):
    a, b, c, d = range(-1, -5, -1)
    s0 = (r_type(n), TYPE, IN, a)
    K = meta["K"]
    return {
        # Q1's shape: rounds {G, H}, {TYPE b, FN_EQ c -> b}, {TYPE c}
        "q1": _plan([s0, (a, P_G, OUT, b), (a, P_H, OUT, c),
                     (b, TYPE, OUT, T_D), (c, P_LD, OUT, b),
                     (c, TYPE, OUT, T_L)], 3),
        # depth-3 ladder: no two ops share a round
        "ladder": _plan([s0, (a, P_G, OUT, b), (b, P_DH, OUT, c),
                         (c, P_EH, OUT, d)], 4),
        # plan order != round order: G2 runs in round 0, before the FN_EQ,
        # and still writes the THIRD column
        "reorder": _plan([s0, (a, P_H, OUT, b), (b, P_BACK, OUT, a),
                          (a, P_G2, OUT, c)], 3),
        # CHAIN_MAX independent ops: 4 rounds of 2
        "ind8": _plan([s0, (a, P_G, OUT, b), (a, TYPE, OUT, T_HALF),
                       (a, P_G2, OUT, c), (a, TYPE, OUT, r_type(NA)),
                       (a, TYPE, OUT, r_type(1025)), (a, P_H, OUT, d),
                       (a, TYPE, OUT, r_type(1024)),
                       (a, TYPE, OUT, r_type(1023))], 4),
        # FN_EQ through the reversed map: the collector swaps the roles
        "rev": _plan([s0, (a, P_G2, OUT, b), (b, P_G, IN, a)], 2),
        # EQ alone in the last round (it reads the column BACK appends);
        # only A[5] survives: L[5] points back at A[6], the subject of K[2]
        "eq-alone": _plan([s0, (a, P_H, OUT, b), (b, P_BACK, OUT, c),
                           (c, P_R, OUT, int(K[2]))], 3),
        # absent append keys: the consumers run a round later, on
        # candidates that are already dead
        "absent": _plan([s0, (a, P_H, OUT, b), (b, TYPE, OUT, T_L),
                         (b, P_BACK, OUT, c)], 3),
        "multi": _plan([s0, (a, P_G, OUT, b), (b, TYPE, OUT, T_X),
                        (b, P_DH, OUT, c)], 3),
        # keep none (every wave leaves after round 0) / all / exactly one
        "none": _plan([s0, (a, TYPE, OUT, T_NONE), (a, P_G, OUT, b),
                       (b, P_DH, OUT, c)], 3),
        "all": _plan([s0, (a, P_G, OUT, b), (a, P_G2, OUT, c),
                      (b, P_DH, OUT, d)], 4),
        "one": _plan([s0, (a, P_G, OUT, b), (a, TYPE, OUT, last_type(n)),
                      (b, P_DH, OUT, c)], 3),
    }


def exp_plans(n, meta):
    a, b, c, d = range(-1, -5, -1)
    s0 = (r_type(n), TYPE, IN, a)
    ex = (a, P_E, OUT, b)
    return {
        # Q7's shape: TYPE and FN_EQ both on the edge value, one round
        "x-q7": _plan([s0, ex, (b, TYPE, OUT, T_C1), (b, P_CA, OUT, a)], 2),
        # the same over two input columns (c = the subject's own label)
        "x-q7-nc2": _plan([s0, (a, P_H, OUT, c), ex, (b, TYPE, OUT, T_C1),
                           (b, P_CL, OUT, c)], 3),
        # trailing appends: the writer walks the rounds APPEND_ONLY
        "x-q7-app": _plan([s0, ex, (b, TYPE, OUT, T_C1), (b, P_CA, OUT, a),
                           (b, P_CL, OUT, c), (a, P_G, OUT, d)], 4),
        # the first op drops every candidate
        "x-none": _plan([s0, ex, (b, TYPE, OUT, T_NONE), (b, P_CL, OUT, c),
                         (c, TYPE, OUT, T_L)], 3),
    }


class Ctx:
    def __init__(self):
        self.triples, self.meta = sched_graph()
        self.ora = OracleCtx(self.triples)
        self.cases = {}
        for n in ROWS:
            for k, p in row_plans(n, self.meta).items():
                self.cases["%s-n%d" % (k, n)] = p
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
# CPU part: the scheduler
# ---------------------------------------------------------------------
SCHED_MAIN = r"""
#include "wk_chain_sched.h"
#include <cstdio>
// stdin, one chain per line: packed nc_in nops {kind a b} x nops
// stdout: nrounds early_out {round_of dst} x nops {slot} x nrounds x SLOTS
int main() {
    static_assert(CHAIN_MAX == %d && CHAIN_SLOTS == %d, "test constants");
    int packed, nc_in, nops;
    while (scanf("%%d %%d %%d", &packed, &nc_in, &nops) == 3) {
        chain_sched_op ops[CHAIN_MAX];
        for (int i = 0; i < nops; i++)
            if (scanf("%%d %%d %%d", &ops[i].kind, &ops[i].a, &ops[i].b) != 3)
                return 1;
        chain_sched S;
        chain_schedule(ops, nops, nc_in, packed != 0, S);
        printf("%%d %%d", S.nrounds, S.early_out);
        for (int i = 0; i < nops; i++)
            printf(" %%d %%d", S.round_of[i], S.dst[i]);
        for (int r = 0; r < S.nrounds; r++)
            for (int s = 0; s < CHAIN_SLOTS; s++) printf(" %%d", S.slot[r][s]);
        printf("\n");
    }
    return 0;
}
""" % (CHAIN_MAX, CHAIN_SLOTS)


def random_chains(seed=7, per_len=150):
    rnd = random.Random(seed)
    out = []
    for nops in range(1, CHAIN_MAX + 1):
        for _ in range(per_len):
            nc_in = rnd.randint(1, 3)
            nc, ops = nc_in, []
            for _i in range(nops):
                kinds = [CH_TYPE, FN_EQ, CH_EQ]
                if nc < 8:
                    kinds += [FN_APPEND] * 3
                k = rnd.choice(kinds)
                # late columns are favoured so that dependencies are common
                pick = lambda: (rnd.randrange(nc) if rnd.random() < 0.5
                                else nc - 1)
                ops.append((k, pick(), pick() if k == FN_EQ else 0))
                if k == FN_APPEND:
                    nc += 1
            out.append((nc_in, ops))
    return out


def test_scheduler_properties(tmp_path):
    src = tmp_path / "sched_main.cpp"
    exe = tmp_path / "sched_main"
    src.write_text(SCHED_MAIN)
    csrc = os.path.join(os.path.dirname(wk_build.__file__), "csrc")
    subprocess.check_call([wk_build.HIPCC, "-std=c++17", "-O1", "-I", csrc,
                           str(src), "-o", str(exe)])
    chains = random_chains()
    lines = []
    for packed in (1, 0):
        for nc_in, ops in chains:
            lines.append(" ".join(
                [str(packed), str(nc_in), str(len(ops))] +
                ["%d %d %d" % o for o in ops]))
    res = subprocess.run([str(exe)], input="\n".join(lines) + "\n",
                         capture_output=True, text=True, check=True)
    got = [list(map(int, ln.split())) for ln in res.stdout.splitlines()]
    assert len(got) == 2 * len(chains)
    shared = 0
    for li, vals in enumerate(got):
        packed = li < len(chains)
        nc_in, ops = chains[li % len(chains)]
        n = len(ops)
        nrounds, early = vals[0], vals[1]
        round_of = vals[2:2 + 2 * n:2]
        dst = vals[3:3 + 2 * n:2]
        slots = vals[2 + 2 * n:]
        assert len(slots) == nrounds * CHAIN_SLOTS
        rounds = [[i for i in slots[r * CHAIN_SLOTS:(r + 1) * CHAIN_SLOTS]
                   if i >= 0] for r in range(nrounds)]
        # every op exactly once, in the round the table says
        assert sorted(i for r in rounds for i in r) == list(range(n))
        assert all(round_of[i] == r for r, ops_r in enumerate(rounds)
                   for i in ops_r)
        assert all(1 <= len(r) <= CHAIN_SLOTS for r in rounds)
        # appends keep their plan-order columns
        nc = nc_in
        for i, (k, a, b) in enumerate(ops):
            if k == FN_APPEND:
                assert dst[i] == nc
                nc += 1
            else:
                assert dst[i] == -1
        # producers strictly earlier
        for i, (k, a, b) in enumerate(ops):
            reads = {a} | ({b} if k == FN_EQ else set())
            for j in range(i):
                if ops[j][0] == FN_APPEND and dst[j] in reads:
                    assert round_of[j] < round_of[i], (ops, round_of)
        if packed:
            assert early == 1 and nrounds <= n
            shared += any(len(r) > 1 for r in rounds)
        else:
            assert early == 0
            assert rounds == [[i] for i in range(n)]
    assert shared > len(chains) // 2        # the packing does pack


# ---------------------------------------------------------------------
# CPU part: the plans
# ---------------------------------------------------------------------
def test_oracle_vs_brute(ctx):
    for name, plan in ctx.cases.items():
        if name.endswith(("-n65", "-n1025")):
            assert _same(ctx.want(name),
                         sort_rows(ctx.ora.brute_query(plan))), name


def test_keep_rates(ctx):
    store = wk.Store(ctx.triples)
    assert store.check() == 0
    A = ctx.meta["A"]
    for p in (P_LD, P_CA):
        k, e = store.seg_stats(p, OUT)
        assert k == e > 0, p                          # functional
    for n in ROWS:
        w = lambda k_: ctx.want("%s-n%d" % (k_, n))
        start = store.get_index(r_type(n), IN)
        assert len(start) == n and int(start[-1]) == int(A[n - 1])
        assert len(w("none")) == 0 == len(w("x-none"))
        assert len(w("all")) == n == len(w("ladder"))
        # exactly one survivor, the last row of the last tile
        assert len(w("one")) == 1 and int(w("one")[0, 0]) == int(A[n - 1])
        assert len(w("eq-alone")) == (1 if n > 5 else 0)
        assert len(w("multi")) == (n + ND - 1) // ND
        assert len(w("rev")) == (n + 7) // 8
        # q % 3 != 0 has a label; of those the even subjects pass FN_EQ
        q = np.arange(n)
        assert len(w("absent")) == int((q % 3 != 0).sum())
        assert len(w("q1")) == int(((q % 3 != 0) & (q % 2 == 0)).sum())
        assert len(w("reorder")) == len(w("q1"))
        assert len(w("ind8")) == int(((q % 3 != 0) & (q % 2 == 0) &
                                      (q < 1023)).sum())
        if n >= 63:
            assert 0 < len(w("q1")) < len(w("absent")) < n
            # the third column of `reorder` is G2's department
            D = ctx.meta["D"]
            r = w("reorder")
            qi = r[:, 0].astype(np.int64) - int(A[0])
            assert np.array_equal(r[:, 2], D[(qi * 3) % ND])
        if n >= 65:
            # first edges of even courses pass; rows of > 32 edges among them
            x = w("x-q7")
            assert 0 < len(x) < n and len(w("x-q7-app")) < len(x)
            assert len(w("x-q7-app")) > 0 and len(w("x-q7-nc2")) > 0
            assert int(A[14]) in set(x[:, 0].tolist())  # 33 edges


# ---------------------------------------------------------------------
# GPU part
# ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine(ctx):
    return wk.Engine(wk.GpuStore(wk.Store(ctx.triples), device=0))


def _run_arm(eng, ctx, names, arm):
    with env(**ARMS[arm]):
        for name in names:
            plan, want = ctx.cases[name], ctx.want(name)
            eng.submit(plan)
            got = sort_rows(eng.fetch_result())
            assert _same(got, want), (name, arm, "submit", got.shape,
                                      want.shape)
            gid = eng.graph_build(plan)
            assert eng.graph_run(gid) == len(want), (name, arm, "replay")
            got = sort_rows(eng.fetch_result(plan))
            assert _same(got, want), (name, arm, "replay", got.shape,
                                      want.shape)


@pytest.mark.gpu
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("arm", list(ARMS))
def test_row_pass_rounds(ctx, engine, arm, n):
    """k_row_chain: every row-pass plan at one start size under one arm,
    through submit and a captured replay."""
    names = ["%s-n%d" % (k, n) for k in row_plans(n, ctx.meta)]
    _run_arm(engine, ctx, names, arm)


@pytest.mark.gpu
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("arm", list(ARMS))
def test_expansion_rounds(ctx, engine, arm, n):
    """k_csr_gather_chain / k_expand_chain over the P_E ladder; under
    WK_CHAIN_GRID=1 one block walks every iteration (>= 3 of them from
    1025 rows on, the last one with clamped rows)."""
    names = ["%s-n%d" % (k, n) for k in exp_plans(n, ctx.meta)]
    _run_arm(engine, ctx, names, arm)
