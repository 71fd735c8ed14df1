"""In-process loopback over the partitions of one graph (a helper module,
not a test).

`PartSet(triples, W)` holds the W partitioned stores of a graph, built
the way the multi-GPU driver builds them (`wk.Store(triples, sid=r,
nsrv=W)`), with one oracle context and, on a GPU, one engine per rank.
`run_plan` walks a plan over W step-level executors the way
`DistQuery._run_steps` of wukong_amd/dist.py does, with the collectives
replaced by plain loops in this one process: an index start runs on
every rank, a constant start on its owner, rows are re-split by
`value % W` before a step whose start variable they are not local by,
and a mid-plan constant/index start filters every rank against the
merged list.  UNION, OPTIONAL and predicate variables are not handled.

The executor is a parameter: `OracleExecutor`s prove the driver on the
CPU before any engine depends on it.
"""
import numpy as np

import wukong_amd as wk
from wukong_amd.dist import (GpuExecutor, filter_rows, plan_v2c_states,
                             _is_tpid)
from tests.oracle_util import OracleCtx, OracleExecutor
from tests.synth_graph import env

MAX_ENGINES = 8


class PartSet:
    """The W partitions of one graph.  Every store gets the FULL triple
    array; wk.Store keeps its share.  `store_env` holds the WK_* values
    set while the stores (and engines) build."""

    def __init__(self, triples, W, store_env=None, oracle=True):
        self.triples, self.W = triples, W
        self.store_env = dict(store_env or {})
        with env(**self.store_env):
            self.stores = [wk.Store(triples, sid=r, nsrv=W) for r in range(W)]
        self.oras = [OracleCtx(triples, sid=r, nsrv=W)
                     for r in range(W)] if oracle else None
        self.gstores, self.engines = None, None

    def build_engines(self, device=0, **engine_env):
        assert self.W <= MAX_ENGINES
        with env(**self.store_env, **engine_env):
            self.gstores = [wk.GpuStore(s, device=device) for s in self.stores]
            self.engines = [wk.Engine(g) for g in self.gstores]
        return self.engines

    def close(self):
        """Drop engines and device stores now (a later PartSet must not
        find them alive)."""
        self.engines = None
        self.gstores = None

    def oracle_executors(self, plan):
        return [OracleExecutor(o, plan) for o in self.oras]

    def engine_executors(self, plan):
        return [GpuExecutor(e, plan) for e in self.engines]


def split_host(table, col, W):
    """Rows of `table` per destination rank: value of `col` modulo W."""
    t = np.asarray(table)
    if t.ndim != 2 or not len(t):
        return [t] * W
    dst = t[:, col] % np.uint32(W)
    return [t[dst == r] for r in range(W)]


def _concat(parts, ncols):
    parts = [p for p in parts if p.ndim == 2 and len(p)]
    if not parts:
        return np.empty((0, ncols), dtype=np.uint32)
    return np.ascontiguousarray(np.concatenate(parts, axis=0))


def exchange_host(exs, col, v2c, ncols, step):
    """fetch, split in numpy, load: works for any executor."""
    W = len(exs)
    for ex in exs:
        ex.rows()                     # resolve an asynchronous filter step
    chunks = [split_host(np.asarray(ex.table()).reshape(-1, ncols), col, W)
              for ex in exs]
    moved = 0
    for dst, ex in enumerate(exs):
        moved += sum(len(chunks[src][dst]) for src in range(W) if src != dst)
        ex.load(_concat([chunks[src][dst] for src in range(W)], ncols),
                v2c, step)
    return moved


def exchange_device(exs, col, v2c, ncols, step):
    """What the all-to-all moves, between engines of one process:
    generate_sub_query packs the per-destination chunks of every rank
    into a device buffer, and each chunk enters its destination engine
    through load_rbuf_device at its offset in that buffer.  The engine
    has no append, so the chunks a destination received are read back
    and loaded as one table."""
    W = len(exs)
    bufs, sizes = [], []
    try:
        for ex in exs:
            n = max(int(ex.rows()), 1)
            buf = wk.dev_alloc((n * ncols + 1) * 4)
            bufs.append(buf)
            sz = [int(x) for x in ex.engine.generate_sub_query(W, buf, n)]
            assert sum(sz) == int(ex.rows()), (sz, ex.rows())
            sizes.append(sz)
        moved = 0
        for dst, ex in enumerate(exs):
            got = []
            for src in range(W):
                n = sizes[src][dst]
                if src != dst:
                    moved += n
                off = sum(sizes[src][:dst])
                ex.engine.load_rbuf_device(bufs[src] + off * ncols * 4, n,
                                           ncols, v2c, step)
                chunk = ex.engine.fetch_raw().reshape(-1, ncols)
                assert len(chunk) == n, (src, dst, len(chunk), n)
                assert n == 0 or (chunk[:, col] % W == dst).all(), (src, dst)
                got.append(chunk)
            ex.load(_concat(got, ncols), v2c, step)
        return moved
    finally:
        for b in bufs:
            wk.dev_free(b)


EXCHANGES = {"host": exchange_host, "device": exchange_device}


def run_plan(exs, plan, exchange="host", trace=None):
    """Run `plan` over the rank-ordered executors `exs` (fresh: at
    pattern 0) and return the concatenated per-rank result tables.
    `exchange` is "host", "device" or None (rows are never re-split:
    wrong on purpose).  `trace`, a dict, receives the number of rows
    that changed rank and the number of list filters."""
    if plan.unions or plan.optional:
        raise ValueError("UNION / OPTIONAL are out of scope for the loopback")
    if plan.distinct or plan.limit >= 0 or plan.offset:
        raise ValueError("final ops would have to run after the merge")
    W = len(exs)
    states = plan_v2c_states(plan)
    local_var = None
    moved = nlist = 0
    for i, (s, p, d, o) in enumerate(plan.patterns):
        if p < 0:
            raise ValueError("predicate variables are out of scope")
        if i == 0:
            if s < 0:
                raise ValueError("the first pattern needs a constant start")
            if _is_tpid(s):
                for ex in exs:
                    ex.step()
                local_var = o                  # members are owned rows
            else:
                v2c, ncols = states[0]
                for r, ex in enumerate(exs):
                    if r == s % W:
                        ex.step()
                    else:
                        ex.load(np.empty((0, ncols), dtype=np.uint32), v2c, 1)
                local_var = None               # edge values: any rank
            continue
        v2c_prev, ncols = states[i - 1]
        if s >= 0:
            lists = [ex.get_index(s, d) if _is_tpid(s)
                     else ex.get_triples(s, p, d) for ex in exs]
            merged = np.unique(np.concatenate(
                [np.asarray(x, dtype=np.uint32) for x in lists]))
            for ex in exs:
                ex.filter_with_list(merged, i, v2c_prev, v2c_prev[-(o + 1)])
            nlist += 1
            continue
        if local_var != s:
            if exchange is not None:
                moved += EXCHANGES[exchange](exs, v2c_prev[-(s + 1)],
                                             v2c_prev, ncols, i)
            local_var = s
        for ex in exs:
            ex.step()
    if plan.filters:
        v2c, _ = states[-1]
        for ex in exs:
            if hasattr(ex, "execute_filter"):
                ex.execute_filter()
            else:
                kept = filter_rows(np.asarray(ex.table()), v2c, plan.filters)
                ex.load(kept, v2c, len(plan.patterns))
    for ex in exs:
        ex.rows()
    parts = [np.asarray(ex.finalize()) for ex in exs]
    if trace is not None:
        trace["moved"], trace["list_filters"] = moved, nlist
    return _concat(parts, len(plan.required_vars))
