#!/usr/bin/env python3
"""bench.py — LUBM Q1-Q7 suite throughput on N MI355X GPUs.

One step = one pass of the 7-query OSDI16-plan suite over the LUBM-2560
synthetic store resident in HBM (BASELINE.json configs[1]).  value =
whole-job queries/sec.  N>1: launched by torch.distributed.run, one rank
per GPU, store partitioned by vid % N, per-step RCCL all-to-allv.

A plain run sets up, warms up, times the K steps and prints the result
line.  --full adds the diagnostic legs (self-parity gates, per-query
latency pass, run-to-run spread, roofline probe, embedded emulator
leg, cpu_baseline); --dump-outputs DIR writes what the last timed step
left behind as DIR/<name>.npy (see dump_outputs).

Env knobs: WK_UNIV (default 2560), and under --full WK_CPU_UNIV
(cpu_baseline sample, default = the workload scale: SAME inputs),
WK_SKIP_CPU_BASELINE=1, WK_SKIP_GATES=1, WK_EMU_EMBED (embedded
emulator queries, 0 = off);
WK_DIST_BACKEND=gloo (single-GPU rehearsal of the N>1 path); the full
knob table (WK_INFLIGHT, WK_GRAPH, WK_FN/CSR/TBM budgets, ...) is in
README.md.
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

os.environ.setdefault("WK_KERNEL_TIMING", "1")

HBM_PEAK_GBS = 8000.0  # MI355X spec (MI355X_MICROARCH.md)


T_START = time.time()


def log(*a):
    print(f"[{time.time() - T_START:6.1f}s]", *a, file=sys.stderr, flush=True)


def pctl(xs, p):
    return float(np.percentile(np.asarray(xs), p)) if xs else None


DUMP_BUDGET_BYTES = 64 << 20  # --dump-outputs writes at most this much
DUMP_SAMPLE_SEED = 20160101


def canonical_table(tbl, budget_bytes):
    """Result tables are multisets (row order depends on atomics), so
    the dumped form is the lexicographically sorted table, as float64
    (u32 ids are exact).  A table over its byte budget is cut to a
    fixed, seeded row sample of the sorted table."""
    a = np.asarray(tbl)
    if a.ndim != 2 or a.size == 0:
        return np.zeros((0, a.shape[1] if a.ndim == 2 else 0), np.float64)
    a = a[np.lexsort(a.T[::-1])]
    max_rows = max(1, budget_bytes // (8 * a.shape[1]))
    if a.shape[0] > max_rows:
        rng = np.random.default_rng(DUMP_SAMPLE_SEED)
        a = a[np.sort(rng.choice(a.shape[0], size=max_rows, replace=False))]
    return a.astype(np.float64)


def dump_outputs(outdir, names, last_table, last_rows, replay):
    """--dump-outputs: the arrays a caller of the timed path can get.

    last_step_<q>_table / last_step_<q>_rows: the final query's device
    table and blind row count exactly as the LAST timed step left them
    (each query of a pass reuses the engine's table buffers, so only
    the pass's final query survives the step).  <q>_table / row_counts:
    one extra untimed pass over the same prepared queries (the captured
    graphs where the timed loop replayed graphs), fetched query by
    query.  Tables are canonicalised by canonical_table(); a query with
    no result rows gets no table file (its zero stands in the counts)."""
    os.makedirs(outdir, exist_ok=True)
    per_table = DUMP_BUDGET_BYTES // (len(names) + 2)
    arrays = {}
    if last_table is not None and last_table.size:
        arrays[f"last_step_{names[-1]}_table"] = canonical_table(
            last_table, per_table)
    if last_rows is not None:
        arrays[f"last_step_{names[-1]}_rows"] = np.array(
            [last_rows], dtype=np.float64)
    counts = []
    for name in names:
        nrows, tbl = replay(name)
        counts.append(nrows)
        if tbl is not None and tbl.size:
            arrays[f"{name}_table"] = canonical_table(tbl, per_table)
    arrays["row_counts"] = np.array(counts, dtype=np.float64)
    total = 0
    for key, arr in arrays.items():
        np.save(os.path.join(outdir, key + ".npy"), arr)
        total += arr.nbytes
    assert total <= DUMP_BUDGET_BYTES, total
    log(f"[dump] {len(arrays)} arrays, {total / 1e6:.1f} MB -> {outdir}")


def cpu_baseline(nuniv_workload, seed, triples=None):
    """Oracle engine (DESIGN.md §4 — 'port' of the reference CPU engine)
    timed on this box's host cores, SAME inputs as the GPU workload
    (LUBM-2560 by default), bounded passes (~10-20 s; build excluded).
    WK_CPU_UNIV overrides the sample scale (debug)."""
    import multiprocessing
    from tests.oracle_util import OracleCtx
    import wukong_amd as wk
    from wukong_amd import queries as Q

    cores = multiprocessing.cpu_count()
    nuniv = int(os.environ.get("WK_CPU_UNIV", str(nuniv_workload)))
    t0 = time.time()
    if triples is None or nuniv != nuniv_workload:
        triples = wk.lubm_gen(nuniv, seed=seed)
    ctx = OracleCtx(triples)
    build_s = time.time() - t0
    # one warm pass, then timed passes until ~10 s (min 1)
    t0 = time.time()
    for plan in Q.ALL.values():
        ctx.run_query(plan, mt=cores)
    warm_s = time.time() - t0
    passes, t0 = 0, time.time()
    while passes == 0 or time.time() - t0 < 10.0:
        for plan in Q.ALL.values():
            ctx.run_query(plan, mt=cores)
        passes += 1
    secs = time.time() - t0
    qps = 7.0 * passes / secs
    return {
        "value": round(qps, 3),
        "unit": "queries/s",
        "cores": cores,
        "kind": "port",
        "sample": (f"LUBM-{nuniv}"
                   + ("" if nuniv == nuniv_workload else
                      f" (workload is LUBM-{nuniv_workload})")
                   + f", same seeded inputs, Q1-Q7 suite x{passes} in "
                     f"{secs:.1f}s, oracle engine (restated reference CPU "
                     f"engine), mt={cores}; oracle build {build_s:.1f}s + "
                     f"warm pass {warm_s:.1f}s excluded"),
    }


def run_emulator_batched(args, store, engines, inflight):
    """Batched emulator: the light templates (A1/A2/A3/A5 — 78/86 of
    the mix) go through wk_engine_submit_light_batch, ONE kernel launch
    per window of queries (one wavefront workgroup each), double-
    buffered across two engines; the heavy templates (A4/A6) batch per
    template through the LDS plan interpreter
    (wk_engine_submit_plan_batch — one wavefront workgroup interprets
    the whole plan, binding table in LDS).  Same mix, same blind
    replies — the batching is engine-side scheduling, not a workload
    change."""
    from collections import deque
    import numpy as np
    import wukong_amd as wk
    from wukong_amd import queries as Q

    rng = np.random.default_rng(7)
    pools = {t: np.asarray(store.get_index(Q.EMU_POOLS[t], wk.DIR_IN),
                           dtype=np.int64)
             for t in Q.EMU_WEIGHTS}
    tnames = list(Q.EMU_WEIGHTS)
    w = np.array([Q.EMU_WEIGHTS[t] for t in tnames], dtype=float)
    w /= w.sum()

    # light = 2-pattern c2u + rdf:type filter (derived from the template)
    light_meta = {}
    for t in tnames:
        p = Q.emu_template(t, 1)
        if len(p.patterns) == 2 and p.patterns[1][1] == Q.TYPE_ID:
            light_meta[t] = (p.patterns[0][1], p.patterns[0][2],
                             p.patterns[1][3])
    light_idx = np.array([tn in light_meta for tn in tnames])

    B = int(os.environ.get("WK_EMU_WINDOW", str(max(inflight, 512))))
    heavy_names = [t for t in tnames if t not in light_meta]
    light_engines = list(engines[:2])
    hv, k = {}, 2
    for t in heavy_names:
        hv[t] = list(engines[k:k + 2]) or [engines[0]]
        k += 2
    # heavy templates run through the LDS plan interpreter, batched per
    # template (wk_engine_submit_plan_batch); subject is per-query
    heavy_plans = {t: Q.emu_template(t, 1 << 17) for t in heavy_names}
    for p in heavy_plans.values():
        p.blind = True

    class Batch:
        __slots__ = ("labels", "subj", "pred", "dirs", "cval", "t_gen",
                     "total", "nlight")

    def make_batch(n):
        b = Batch()
        ti = rng.choice(len(tnames), size=n, p=w)
        subj = np.empty(n, np.int64)
        pred = np.empty(n, np.int32)
        dirs = np.empty(n, np.int32)
        cval = np.empty(n, np.uint32)
        heavy = []
        lmask = light_idx[ti]
        for k, tn in enumerate(tnames):
            mask = ti == k
            m = int(mask.sum())
            if not m:
                continue
            consts = pools[tn][rng.integers(0, len(pools[tn]), m)]
            if tn in light_meta:
                pr, dr, cv = light_meta[tn]
                subj[mask] = consts
                pred[mask] = pr
                dirs[mask] = dr
                cval[mask] = cv
            else:
                heavy.append((tn, consts))
        b.labels = [tnames[i] for i in ti[lmask]]
        b.subj, b.pred = subj[lmask], pred[lmask]
        b.dirs, b.cval = dirs[lmask], cval[lmask]
        b.total, b.nlight = n, int(lmask.sum())
        return b, heavy

    def run(total, collect=None):
        produced = 0
        pending = deque()
        free_light = deque(light_engines)
        free_heavy = {t: deque(hv[t]) for t in heavy_names}
        acc = {t: [] for t in heavy_names}    # accumulated consts arrays
        accg = {t: [] for t in heavy_names}   # their gen times
        rerun = [0]

        def harvest_one():
            kind, e, payload = pending.popleft()
            if kind == "light":
                b = payload
                e.wait_light_batch()
                now = time.time()
                if collect is not None:
                    ms = (now - b.t_gen) * 1e3
                    for tn in b.labels:
                        collect.setdefault(tn, []).append(ms)
                free_light.append(e)
            else:
                tn, consts, gens = payload
                counts = e.wait_light_batch()
                for j in np.nonzero(counts == np.uint64(wk.LP_OVERFLOW))[0]:
                    p = Q.emu_template(tn, int(consts[j]))
                    p.blind = True
                    e.run_query_count(p)
                    rerun[0] += 1
                now = time.time()
                if collect is not None:
                    for tg, m in gens:
                        ms = (now - tg) * 1e3
                        collect.setdefault(tn, []).extend([ms] * m)
                free_heavy[tn].append(e)

        while produced < total or pending or any(acc[t] for t in heavy_names):
            progress = False
            if produced < total and free_light:
                tg = time.time()
                b, heavy = make_batch(min(B, total - produced))
                produced += b.total
                for tn, consts in heavy:
                    acc[tn].append(consts)
                    accg[tn].append((tg, len(consts)))
                if b.nlight:
                    e = free_light.popleft()
                    e.submit_light_batch(b.subj, b.pred, b.dirs, b.cval)
                    b.t_gen = tg
                    pending.append(("light", e, b))
                progress = True
            for tn in heavy_names:
                if acc[tn] and free_heavy[tn]:
                    e = free_heavy[tn].popleft()
                    consts = np.concatenate(acc[tn])
                    gens = accg[tn]
                    acc[tn], accg[tn] = [], []
                    e.submit_plan_batch(heavy_plans[tn], consts)
                    pending.append(("heavy", e, (tn, consts, gens)))
                    progress = True
            if pending and (not progress or len(pending) >= 6):
                harvest_one()
        return rerun[0]

    # gate: store must support the fast paths (single-type index +
    # interpretable heavy templates); otherwise per-query emulator
    try:
        probe, _ = make_batch(4)
        if probe.nlight:
            light_engines[0].submit_light_batch(probe.subj, probe.pred,
                                                probe.dirs, probe.cval)
            light_engines[0].wait_light_batch()
        for tn in heavy_names:
            hv[tn][0].submit_plan_batch(heavy_plans[tn],
                                        pools[tn][:2].astype(np.int64))
            hv[tn][0].wait_light_batch()
    except ValueError:
        return False

    run(max(args.emu // 10, 4 * B))  # warmup
    lat = {}
    t0 = time.time()
    nrerun = run(args.emu, collect=lat)
    elapsed = time.time() - t0
    latency = {t: {"p50_ms": round(pctl(xs, 50), 3),
                   "p99_ms": round(pctl(xs, 99), 3), "n": len(xs)}
               for t, xs in sorted(lat.items())}
    return {
        "metric": "light-mix queries/sec (emulator A1-A6, mix_config weights)",
        "value": round(args.emu / elapsed, 1),
        "unit": "queries/s",
        "n_gpus": 1,
        "queries": args.emu,
        "inflight": 2 * B,
        "window": B,
        "mode": "batched (one launch per window, wavefront/query; "
                "heavy templates via LDS plan interpreter)",
        "plan_batch_overflow_reruns": nrerun,
        "higher_is_better": True,
        "dtype": "u32",
        "data": "synthetic",
        "config": {"workload": "LUBM-2560 light-template mix, blind replies "
                               "(proxy.hpp:491), batched in-flight window "
                               "(proxy.hpp:477-525)"},
        "latency": latency,
    }


def run_emulator(args, store, engines, inflight):
    """The reference's sparql-emu benchmark (Proxy::run_query_emu,
    core/proxy.hpp:391-545): light templates A1-A6 with mix_config
    weights, %-constants drawn from type-index candidates, `-p`-style
    in-flight window, blind replies; reports qps + per-type p50/p99."""
    import random
    from collections import deque
    import wukong_amd as wk
    from wukong_amd import queries as Q

    rng = random.Random(7)
    pools = {t: store.get_index(Q.EMU_POOLS[t], wk.DIR_IN)
             for t in Q.EMU_WEIGHTS}
    tnames = list(Q.EMU_WEIGHTS)
    weights = [Q.EMU_WEIGHTS[t] for t in tnames]

    def gen_query():
        t = rng.choices(tnames, weights)[0]
        c = int(rng.choice(pools[t]))
        p = Q.emu_template(t, c)
        p.blind = True
        return t, p

    def harvest(eng_, plan_):
        n = eng_.fetch_count()
        while n < 0:
            eng_.submit(plan_)
            n = eng_.fetch_count()
        return n

    nthreads = int(os.environ.get("WK_EMU_THREADS", "6"))
    nthreads = max(1, min(nthreads, len(engines)))

    def run_window(engs, n, seed, collect=None):
        # one submitter's pipeline over its engine subset (ctypes releases
        # the GIL inside submit/fetch, so threads overlap on the host too)
        lrng = random.Random(seed)
        pending = deque()
        free = list(engs)

        def gen_q():
            t = lrng.choices(tnames, weights)[0]
            c = int(lrng.choice(pools[t]))
            p = Q.emu_template(t, c)
            p.blind = True
            return t, p

        for _ in range(n):
            if not free:
                t_, e_, ti_, p_ = pending.popleft()
                harvest(e_, p_)
                if collect is not None:
                    collect.setdefault(t_, []).append((time.time() - ti_) * 1e3)
                free.append(e_)
            t, p = gen_q()
            e_ = free.pop()
            ti = time.time()
            e_.submit(p)
            pending.append((t, e_, ti, p))
        while pending:
            t_, e_, ti_, p_ = pending.popleft()
            harvest(e_, p_)
            if collect is not None:
                collect.setdefault(t_, []).append((time.time() - ti_) * 1e3)

    def run(n, collect=None):
        import threading
        chunks = [engines[i::nthreads] for i in range(nthreads)]
        per = n // nthreads
        cols = [dict() for _ in range(nthreads)]
        ths = [threading.Thread(target=run_window,
                                args=(chunks[i], per, 100 + i,
                                      cols[i] if collect is not None else None))
               for i in range(nthreads)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        if collect is not None:
            for c in cols:
                for k, v in c.items():
                    collect.setdefault(k, []).extend(v)

    run(max(args.emu // 10, inflight * 2))  # warmup
    lat = {}
    t0 = time.time()
    run(args.emu, collect=lat)
    elapsed = time.time() - t0
    latency = {t: {"p50_ms": round(pctl(xs, 50), 3),
                   "p99_ms": round(pctl(xs, 99), 3), "n": len(xs)}
               for t, xs in sorted(lat.items())}
    out = {
        "metric": "light-mix queries/sec (emulator A1-A6, mix_config weights)",
        "value": round(args.emu / elapsed, 1),
        "unit": "queries/s",
        "n_gpus": 1,
        "queries": args.emu,
        "inflight": inflight,
        "submit_threads": nthreads,
        "higher_is_better": True,
        "dtype": "u32",
        "data": "synthetic",
        "config": {"workload": "LUBM-2560 light-template mix, blind replies "
                               "(proxy.hpp:491), in-flight window "
                               "(proxy.hpp:477-525)"},
        "latency": latency,
    }
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # default steps size the timed region to >= 1 s (~0.9 ms/pass)
    ap.add_argument("--steps", type=int, default=1500)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--watdiv", type=int, default=0,
                    help="WatDiv mode: generate N products (~55N triples) and "
                         "run the star/linear/snowflake templates instead of "
                         "the LUBM suite")
    ap.add_argument("--emu", type=int, default=0,
                    help="emulator light-mix mode: run N template queries "
                         "(A1-A6, mix_config weights) through the in-flight "
                         "window; reports its own JSON line")
    ap.add_argument("--full", action="store_true",
                    help="also run the diagnostic legs: self-parity gates, "
                         "per-query latency pass, run-to-run spread, roofline "
                         "probe, embedded emulator leg, cpu_baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed "
                         "step computed as DIR/<name>.npy (float64, <= 64 MB)")
    args = ap.parse_args()

    # no benchmark plan (LUBM Q1-Q7, emulator A1-A6, WatDiv templates)
    # has a predicate variable, so the per-vertex predicate lists that
    # only such plans read are not built or uploaded (WK_VERSATILE=1
    # brings them back)
    os.environ.setdefault("WK_VERSATILE", "0")

    import wukong_amd as wk
    from wukong_amd import queries as Q

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    if os.environ.get("WK_DIST_BACKEND") == "gloo":
        import torch as _t
        local_rank = local_rank % max(_t.cuda.device_count(), 1)
    ngpus = max(args.gpus, world)
    distributed = world > 1

    seed = 42
    nuniv = int(os.environ.get("WK_UNIV", "2560"))
    dataset = f"LUBM-{nuniv}"
    if args.watdiv:
        dataset = f"WatDiv-{args.watdiv}p"

    if distributed:
        import torch
        import torch.distributed as dist
        # WK_DIST_BACKEND=gloo: single-GPU rehearsal of the full N>1
        # code path (host exchanges; RCCL refuses 2 ranks on 1 device)
        backend = os.environ.get("WK_DIST_BACKEND", "nccl")
        torch.cuda.set_device(local_rank % max(torch.cuda.device_count(), 1))
        dist.init_process_group(backend)
        from wukong_amd.dist import DistQuery, GpuExecutor

    t0 = time.time()
    if args.watdiv:
        triples = wk.watdiv_gen(args.watdiv, seed=seed, sid=rank, nsrv=world)
    else:
        triples = wk.lubm_gen(nuniv, seed=seed, sid=rank, nsrv=world)
    log(f"[rank {rank}] gen {dataset}: {triples.shape[0]} triples "
        f"({time.time()-t0:.1f}s)")
    t0 = time.time()
    store = wk.Store(triples, sid=rank, nsrv=world)
    # the cpu_baseline leg reuses the SAME generated inputs (north_star:
    # reference CPU engine timed on the same inputs)
    keep_triples = (args.full and not distributed and not args.watdiv
                    and os.environ.get("WK_SKIP_CPU_BASELINE") != "1"
                    and int(os.environ.get("WK_CPU_UNIV", str(nuniv))) == nuniv)
    if not keep_triples:
        del triples
        triples = None
    log(f"[rank {rank}] store: {store.num_slots} slots, {store.num_edges} edges "
        f"({time.time()-t0:.1f}s)")
    t0 = time.time()
    # heavy queries keep their tables L3-resident; concurrent engines evict
    # each other (measured: inflight=8 halves throughput at LUBM-2560), so
    # the headline run is sequential; WK_INFLIGHT>1 suits light-query mixes
    inflight = 1 if distributed else int(
        os.environ.get("WK_INFLIGHT", "16" if args.emu else "1"))
    gstore = wk.GpuStore(store, device=local_rank)
    engines = [wk.Engine(gstore, device=local_rank) for _ in range(inflight)]
    eng = engines[0]
    log(f"[rank {rank}] HBM upload {((store.num_slots*16+store.num_edges*4)/1e9):.2f} GB, "
        f"{inflight} engine(s) ({time.time()-t0:.1f}s)")
    if distributed:
        # xGMI peer mappings: sub-threshold steps read the owner's store
        # in place instead of exchanging (dist.py init_peers; falls back
        # to exchange-only on any rank's failure, uniformly)
        from wukong_amd.dist import init_peers
        peers_ok = init_peers(gstore, store)
        log(f"[rank {rank}] xGMI peer mappings: "
            f"{'ok' if peers_ok else 'unavailable (exchange-only)'}")

    if args.watdiv:
        from wukong_amd import watdiv as W
        Q_ALL = W.ALL
    else:
        Q_ALL = Q.ALL
    names = list(Q_ALL)

    if args.emu and not distributed:
        if os.environ.get("WK_EMU_MODE", "batched") == "batched":
            rec = run_emulator_batched(args, store, engines, inflight)
            if rec:
                print(json.dumps(rec), flush=True)
                return
        run_emulator(args, store, engines, inflight)
        return

    def harvest(eng_, plan_):
        n = eng_.fetch_count()
        while n < 0:  # capacity grew; resubmit (overflow re-run)
            eng_.submit(plan_)
            n = eng_.fetch_count()
        return n

    graph_ids = {}  # plan name -> captured hipGraph id (single-GPU path)

    def build_graphs():
        """Capture each suite plan as a hipGraph after warmup (the
        launch chain replays in ONE hipGraphLaunch).  WK_GRAPH=0
        disables; any per-plan failure falls back to submit."""
        if distributed or os.environ.get("WK_GRAPH", "1") == "0":
            return
        for name in names:
            try:
                graph_ids[name] = eng.graph_build(Q_ALL[name])
            except Exception as ex:  # fall back silently to submit path
                log(f"[graph] {name}: fallback to submit ({ex})")

    def run_suite(collect=None, passes=1):
        """Distributed path / single-engine fallback: sequential queries."""
        for _ in range(passes):
            for name in names:
                plan = Q_ALL[name]
                tq = time.time()
                if distributed:
                    ex = GpuExecutor(eng, plan)
                    dq = DistQuery(ex, plan, rank, world,
                                   device=f"cuda:{local_rank}")
                    dq.run()
                    part = eng.fetch_count()  # blind reply (proxy.hpp:491)
                    cnt = torch.tensor([part], dtype=torch.int64,
                                       device=f"cuda:{local_rank}")
                    dist.all_reduce(cnt)
                    nrows = int(cnt.item())
                elif name in graph_ids:
                    try:
                        nrows = eng.graph_run(graph_ids[name])
                    except OverflowError:
                        del graph_ids[name]
                        nrows = eng.run_query_count(plan)
                else:
                    nrows = eng.run_query_count(plan)
                if collect is not None:
                    collect.setdefault(name, []).append((time.time() - tq) * 1e3)
                    collect.setdefault("_rows", {})[name] = nrows

    def run_pipelined(passes, collect=None):
        """In-flight window over engine pool — the reference proxy's
        emulator mode (`-p`, core/proxy.hpp:477-525), blind replies."""
        from collections import deque
        pending = deque()
        free = list(engines)
        seq = [name for _ in range(passes) for name in names]

        def drain_one():
            name_, eng_, t_iss, plan_ = pending.popleft()
            n = harvest(eng_, plan_)
            if collect is not None:
                collect.setdefault(name_, []).append((time.time() - t_iss) * 1e3)
                collect.setdefault("_rows", {})[name_] = n
            free.append(eng_)

        for name in seq:
            if not free:
                drain_one()
            eng_ = free.pop()
            plan = Q_ALL[name]
            t_iss = time.time()
            eng_.submit(plan)
            pending.append((name, eng_, t_iss, plan))
        while pending:
            drain_one()

    def device_sync():
        # whole-device sync on this rank's GPU, straight from the HIP
        # runtime the engine library links (a single-GPU run never
        # needs torch, whose import and context cost seconds of setup)
        if distributed:
            torch.cuda.synchronize(local_rank)
            return
        hip = wk._lib
        if hip.hipSetDevice(local_rank) or hip.hipDeviceSynchronize():
            raise RuntimeError("hipDeviceSynchronize failed")

    def sync():
        device_sync()
        if distributed:
            dist.barrier()
            device_sync()

    def all_stats():
        tot = {}
        for en in engines:
            for k, v in en.kernel_stats().items():
                t = tot.setdefault(k, dict(usec=0.0, bytes=0.0, launches=0))
                t["usec"] += v["usec"]
                t["bytes"] += v["bytes"]
                t["launches"] += v["launches"]
        return tot

    # warmup
    log(f"[rank {rank}] warmup...")
    if distributed or inflight == 1:
        run_suite(passes=args.warmup)
        build_graphs()
        run_suite(passes=1)  # one graph-mode warm pass
    else:
        run_pipelined(args.warmup)
    sync()

    # at-scale self-parity gates (the gsck idea, gchecker.hpp:364-392):
    # store integrity scan + per-query counts must agree between the
    # functional-map and classic dispatch paths AND between graph replay
    # and submit — asserted on the full workload store (--full runs)
    gates = None
    if (args.full and not distributed
            and os.environ.get("WK_SKIP_GATES") != "1"):
        t0 = time.time()
        viol = store.check()
        if viol:
            raise RuntimeError(f"parity gate: store check violations={viol}")
        gate_counts = {}
        for name in names:
            plan = Q_ALL[name]
            n_fn = eng.run_query_count(plan)
            os.environ["WK_FN_DISPATCH"] = "0"
            try:
                n_classic = eng.run_query_count(plan)
            finally:
                os.environ.pop("WK_FN_DISPATCH", None)
            if n_fn != n_classic:
                raise RuntimeError(
                    f"parity gate: {name} fn-dispatch {n_fn} != classic "
                    f"{n_classic}")
            if name in graph_ids:
                n_graph = eng.graph_run(graph_ids[name])
                if n_graph != n_fn:
                    raise RuntimeError(
                        f"parity gate: {name} graph {n_graph} != submit {n_fn}")
            gate_counts[name] = n_fn
        gates = {"store_check": "ok", "counts": gate_counts,
                 "paths": "fn==classic" + ("==graph" if graph_ids else ""),
                 "secs": round(time.time() - t0, 1)}
        log(f"[gates] ok: {gates}")
        sync()
    stats0 = all_stats()

    lat = {}
    # full graph coverage: per-query latencies from a dedicated
    # sequential pass (--full), then the TIMED loop enqueues all replays
    # of a pass back-to-back with ONE sync (the reference proxy's
    # in-flight window applied to replays; graphs serialize safely on
    # one stream)
    graphs_all = (not distributed and inflight == 1
                  and all(n in graph_ids for n in names))
    suite_gid = None
    if graphs_all:
        if args.full:
            run_suite(collect=lat, passes=3)
        try:
            # whole-pass capture: ONE instantiated graph for all 7
            # queries -> the graph-replay floor is paid once per pass
            suite_gid = eng.graph_build_suite([Q_ALL[n] for n in names])
        except Exception as ex:
            log(f"[graph] suite capture fallback ({ex})")
    log(f"[rank {rank}] timed region: {args.steps} steps...")
    t_start = time.time()
    if graphs_all:
        try:
            for _ in range(args.steps):
                if suite_gid is not None:
                    eng.graph_launch(suite_gid)
                else:
                    for name in names:
                        eng.graph_launch(graph_ids[name])
                eng.sync()
        except OverflowError:
            log("[graph] pipelined replay overflow: classic timed loop")
            graphs_all = False
            t_start = time.time()
            run_suite(collect=lat, passes=args.steps)
    elif distributed or inflight == 1:
        run_suite(collect=lat, passes=args.steps)
    else:
        run_pipelined(args.steps, collect=lat)
    sync()
    elapsed = time.time() - t_start
    stats1 = all_stats()

    if args.dump_outputs and rank == 0:
        single = not distributed and inflight == 1
        # the single-engine loops leave the pass's final query resident
        last_table = eng.fetch_raw() if single else None
        last_rows = (last_table.shape[0] if single
                     else lat.get("_rows", {}).get(names[-1]))

        def replay(name):
            if not single:  # counts of the last timed pass; no tables
                return lat.get("_rows", {}).get(name, -1), None
            nrows = None
            if name in graph_ids:
                try:
                    nrows = eng.graph_run(graph_ids[name])
                except OverflowError:
                    pass
            if nrows is None:
                nrows = eng.run_query_count(Q_ALL[name])
            return nrows, eng.fetch_raw()

        dump_outputs(args.dump_outputs, names, last_table, last_rows, replay)

    # run-to-run spread: repeat the identical timed region (diagnostic
    # only — `value` comes from the official K-step region above)
    spread = None
    if args.full and graphs_all and elapsed < 5.0:
        reps = [elapsed]
        for _ in range(2):
            t0 = time.time()
            for _ in range(args.steps):
                if suite_gid is not None:
                    eng.graph_launch(suite_gid)
                else:
                    for name in names:
                        eng.graph_launch(graph_ids[name])
                eng.sync()
            sync()
            reps.append(time.time() - t0)
        spread = {"region_s": [round(r, 4) for r in reps],
                  "pct": round(100 * (max(reps) - min(reps)) / min(reps), 2)}

    if distributed:
        t = torch.tensor([elapsed], dtype=torch.float64,
                         device=f"cuda:{local_rank}")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    if rank != 0:
        if distributed:
            dist.destroy_process_group()
        return

    total_queries = len(names) * args.steps  # 7 LUBM / 5 WatDiv templates
    qps = total_queries / elapsed

    # roofline: dedicated measurement of the dominant kernels on the
    # workload's largest single step (Q1's 6.4M-row known_to_unknown):
    # algorithmic bytes (device-counted) / HIP-event launch time
    def roofline_probe():
        if distributed or not args.full:
            return {}, {}, {}, {}
        if args.watdiv:
            return {}, {}, {}, {}

        def run_steps(e0):
            e0.begin_query(Q.ALL["q1"])
            e0.execute_one_pattern()           # i2u (6.4M grad students)
            e0.execute_one_pattern()           # k2u memberOf
            s0 = e0.kernel_stats()
            e0.execute_one_pattern()           # k2u ugDegreeFrom (the largest
            s1 = e0.kernel_stats()             # expansion launch: 6.4M x 3 cols)
            e0.fetch_count()
            def delta(cat):
                du = s1[cat]["usec"] - s0[cat]["usec"]
                db = s1[cat]["bytes"] - s0[cat]["bytes"]
                dn = s1[cat]["launches"] - s0[cat]["launches"]
                return {"usec": round(du, 1), "bytes": db, "launches": dn,
                        "gbs": round(db / du / 1e3, 1) if du > 0 else None}
            return delta

        e0 = engines[0]
        # classic probe+scan+expand pipeline (the cluster-hash layout
        # of record; diagnostic arm, WK_FN_DISPATCH=0)
        os.environ["WK_FN_DISPATCH"] = "0"
        try:
            d = run_steps(e0)
            rl_expand, rl_probe = d("expand"), d("probe")
        finally:
            os.environ.pop("WK_FN_DISPATCH", None)
        # rank-compressed functional-map path (the production path for
        # this step): 16-B page + 4-B value gather replaces the probe
        d2 = run_steps(e0)
        rl_fn = d2("expand")
        # rank-compressed CSR side-index probe (production path for
        # NON-functional predicates): q7's advisor expansion,
        # 1.5M rows -> 24-B probes via k_csr_gather + k_scan_local
        e0.begin_query(Q.ALL["q7"])
        e0.execute_one_pattern()           # i2u full professors
        s0 = e0.kernel_stats()
        e0.execute_one_pattern()           # k2u advisor (CSR probe)
        s1 = e0.kernel_stats()
        e0.fetch_count()
        du = s1["probe"]["usec"] - s0["probe"]["usec"]
        db = s1["probe"]["bytes"] - s0["probe"]["bytes"]
        rl_csr = {"usec": round(du, 1), "bytes": db,
                  "launches": s1["probe"]["launches"] - s0["probe"]["launches"],
                  "gbs": round(db / du / 1e3, 1) if du > 0 else None}
        return rl_expand, rl_probe, rl_fn, rl_csr

    rl_expand, rl_probe, rl_fn, rl_csr = roofline_probe()
    dk = "expand"
    d_us = stats1[dk]["usec"] - stats0[dk]["usec"]
    d_by = stats1[dk]["bytes"] - stats0[dk]["bytes"]
    d_n = stats1[dk]["launches"] - stats0[dk]["launches"]
    achieved = rl_expand.get("gbs") if rl_expand else None
    if achieved is None and d_us > 0:
        achieved = d_by / d_us / 1e3
    traffic = None
    tj = os.path.join(HERE, "profiles", "traffic.json")
    if os.path.exists(tj):
        with open(tj) as f:
            tdata = json.load(f)
        traffic = tdata.get("expand_bytes_per_launch")
    roofline = {
        "bound": "hbm",
        "kernel": "k_expand",
        "achieved": round(achieved, 1) if achieved else None,
        "peak": HBM_PEAK_GBS,
        "unit": "GB/s",
        "frac": round(achieved / HBM_PEAK_GBS, 4) if achieved else None,
        "traffic": traffic,
        "launches": int(d_n),
        "avg_launch_us": round(d_us / d_n, 2) if d_n else None,
        "measured_on": "Q1 known_to_unknown(ugDegreeFrom), 6.4M rows -> 3 "
                       "cols, LUBM-2560 (largest expansion launch; classic "
                       "probe+scan+expand pipeline, WK_FN_DISPATCH=0 — the "
                       "production path for non-functional predicates)"
                       if rl_expand else "category aggregate",
        "probe_kernel": rl_probe or None,
        # same step through the rank-compressed functional map (submit
        # path: k_fn_gather + k_fn_compact; the graph replay runs the
        # 1:1 k_expand_fn_map at ~5-6 TB/s): algorithmic bytes are
        # 148->28 per row, so GB/s reads lower while wall time is lower
        "fn_map_kernel": rl_fn or None,
        # non-functional-segment probes through the rank-compressed CSR
        # side index (q7 advisor step; the production path for
        # takesCourse/advisor/pubAuthor expansions)
        "csr_probe_kernel": rl_csr or None,
    }

    # embedded emulator leg (driver-reproducible evidence for the
    # light-mix claim): short batched run on the same resident store,
    # reported inside THIS json line.  WK_EMU_EMBED=0 disables.
    emu_rec = None
    n_emu = int(os.environ.get("WK_EMU_EMBED", "200000"))
    if args.full and not distributed and not args.watdiv and n_emu > 0:
        import types
        log("[rank 0] embedded emulator leg...")
        emu_engines = [wk.Engine(gstore, device=local_rank) for _ in range(6)]
        try:
            emu_rec = run_emulator_batched(
                types.SimpleNamespace(emu=n_emu), store, emu_engines, 512)
            if emu_rec is False:
                emu_rec = None
        finally:
            del emu_engines

    cb = None
    if (args.full and os.environ.get("WK_SKIP_CPU_BASELINE") != "1"
            and not distributed and not args.watdiv):
        log("[rank 0] timing cpu_baseline (oracle engine, same inputs)...")
        cb = cpu_baseline(nuniv, seed, triples=triples)
    del triples

    latency = {}
    for name in names:
        xs = lat.get(name, [])
        latency[name] = {"p50_ms": round(pctl(xs, 50), 3) if xs else None,
                         "p99_ms": round(pctl(xs, 99), 3) if xs else None,
                         "rows": lat.get("_rows", {}).get(name)}

    out = {
        "metric": ("queries/sec, WatDiv star/linear/snowflake templates"
                   if args.watdiv else
                   "queries/sec, LUBM-2560 Q1-Q7 mix (OSDI16 plans)"),
        "value": round(qps, 3),
        "unit": "queries/s",
        "n_gpus": ngpus,
        "steps": args.steps,
        "warmup": args.warmup,
        "full": args.full,
        "ms_per_step": round(elapsed * 1e3 / args.steps, 3),
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "u32",
        "data": "synthetic",
        "config": {
            "workload": (f"{dataset} on 1xMI355X, full graph in HBM, "
                         + ("star/linear/snowflake templates"
                            if args.watdiv else "Q1-Q7 mixed light/heavy"))
                        if ngpus == 1 else
                        f"{dataset} subject-hash-partitioned across "
                        f"{ngpus}xMI355X, RCCL all-to-all sub-query shipping",
            "dataset": dataset,
            "queries": ("watdiv templates" if args.watdiv
                        else "lubm q1-q7, osdi16 plans"),
            "blind": True,  # reference emulator semantics, proxy.hpp:491
            "parallelism": f"graph-partitioned x{ngpus} + per-step all-to-allv",
            "inflight": inflight,  # reference emulator window (proxy.hpp -p)
        },
        "timed_region_s": round(elapsed, 4),
        "spread": spread,
        "parity_gates": gates,
        "roofline": roofline,
        "cpu_baseline": cb,
        "emulator": emu_rec,
        "latency": latency,
        "kernel_stats": {k: {"usec": round(stats1[k]["usec"] - stats0[k]["usec"], 1),
                             "launches": int(stats1[k]["launches"] - stats0[k]["launches"])}
                         for k in stats1},
    }
    print(json.dumps(out), flush=True)
    log("[rank 0] result line printed")
    if distributed:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
