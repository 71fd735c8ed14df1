"""A/B of the final ops (DISTINCT / OFFSET / LIMIT): device pass against
the host path (WK_DEV_FINAL=0, read per call), alternated in one process.

Usage: python tools/finalbench.py [--univ=2560] [--reps=20] [--runs=3]
                                  [--only=a] [--out=FILE.json]

Cases: (a) Q2 required=[X] DISTINCT, (b) Q7 DISTINCT, (c) Q2 LIMIT 1000
OFFSET 1000 — whole run_query, p50 over --reps; (d) DISTINCT of an
injected 3-column table of 1,000 and of 100,000 rows — fetch_result alone
(the table is loaded and synced before the clock starts).  Prints one JSON
line; every run of both arms is in it.
"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import wukong_amd as wk  # noqa: E402
from wukong_amd import Plan, queries as Q  # noqa: E402


def opt(name, default):
    for a in sys.argv[1:]:
        if a.startswith("--%s=" % name):
            return a.split("=", 1)[1]
    return default


def p50(fn, reps, prep=None):
    ts = []
    for _ in range(reps):
        if prep:
            prep()   # outside the clock: a fresh table for every fetch
        t = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t))
    return float(np.median(ts))


def main():
    univ, reps, runs = int(opt("univ", 2560)), int(opt("reps", 20)), int(opt("runs", 3))
    only = opt("only", "")
    t0 = time.time()
    triples = wk.lubm_gen(univ, seed=42)
    store = wk.Store(triples)
    del triples
    eng = wk.Engine(store, device=0)
    print(f"setup {time.time() - t0:.1f}s", file=sys.stderr, flush=True)

    cases = {}
    plans = {
        "a_q2_distinct_x": Plan(Q.Q2.patterns, 2, [Q.X], distinct=True),
        "b_q7_distinct": Plan(Q.Q7.patterns, 3, [Q.X, Q.Y, Q.Z], distinct=True),
        "c_q2_limit_offset": Plan(Q.Q2.patterns, 2, [Q.X, Q.Y], limit=1000,
                                  offset=1000),
    }
    for name, plan in plans.items():
        cases[name] = (lambda plan=plan: eng.run_query(plan))
    rng = np.random.default_rng(5)
    inj = Plan([(Q.COURSE, Q.TYPE_ID, wk.DIR_IN, -1)], 3, [-1, -2, -3],
               distinct=True)
    for n in (1000, 100000):
        # ids the size of LUBM's (28 bits), a third of the rows duplicated
        tbl = rng.integers(1 << 17, 1 << 28, size=(n, 3), dtype=np.uint64)
        tbl[n // 3 * 2:] = tbl[:n - n // 3 * 2]
        tbl = tbl.astype(np.uint32)

        def fetch(tbl=tbl):
            eng.fetch_result(inj)

        def prep(tbl=tbl):
            eng.begin_query(inj)
            eng.load_rbuf(tbl, [0, 1, 2], step=1)
            eng.row_count()
        cases["d_inject_%d" % n] = (fetch, prep)

    out = {"univ": univ, "reps": reps, "runs": runs, "cases": {}}
    for name, c in cases.items():
        if only and not name.startswith(only):
            continue
        fn, prep = c if isinstance(c, tuple) else (c, None)
        rec = {"host_ms": [], "device_ms": []}
        for arm in ("0", "1"):                     # warm both arms
            os.environ["WK_DEV_FINAL"] = arm
            if prep:
                prep()
            fn()
        rec["rows"] = int(eng.final_count())
        if name[0] in "ab":
            rec["blind_rows"] = int(eng.run_query_count(plans[name]))
            eng.run_query(plans[name])
            rec["digit_passes_live_total"] = list(eng.final_passes())
        for _ in range(runs):
            for arm, key in (("0", "host_ms"), ("1", "device_ms")):
                os.environ["WK_DEV_FINAL"] = arm
                rec[key].append(round(p50(fn, reps, prep), 4))
        os.environ.pop("WK_DEV_FINAL", None)
        out["cases"][name] = rec
        print(name, rec, file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    path = opt("out", "")
    if path:
        with open(path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
