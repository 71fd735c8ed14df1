#!/usr/bin/env python
"""A/B of UNION / OPTIONAL plans: host merge against the device chain.

Four LUBM group shapes (UNION, OPTIONAL, two-pattern OPTIONAL, UNION +
OPTIONAL), three arms, alternated round by round in one process:
  host   WK_DEV_GROUPS=0, run_query     (host merge, a sync per pattern)
  dev    WK_DEV_GROUPS=1, run_query     (one launch chain)
  graph  graph_run of the captured plan (blind count, no download)
Blind (count-only) plans, so the arms differ in how the groups run, not
in a result download they share.  Prints one JSON record: per shape and
arm the median, min and max wall time in microseconds, and the rows.

  python tools/groups_ab.py --univ 2560 --reps 30 > profiles/bench_groups_ab.json
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import wukong_amd as wk                      # noqa: E402
from wukong_amd import Plan, queries as Q    # noqa: E402

X, Y, Z = -1, -2, -3


def plans():
    grad = (Q.GRADSTUDENT, Q.TYPE_ID, wk.DIR_IN, X)
    ug = (Q.UGSTUDENT, Q.TYPE_ID, wk.DIR_IN, X)
    unions = [[(X, Q.MEMBEROF, wk.DIR_OUT, Y)], [(X, Q.UGDEGREE, wk.DIR_OUT, Y)]]
    return {
        "union": Plan([grad], 2, [X, Y], unions=unions, blind=True),
        "opt": Plan([ug], 2, [X, Y], blind=True,
                    optional=[(X, Q.ADVISOR, wk.DIR_OUT, Y)]),
        "opt2": Plan([ug], 2, [X, Y], blind=True,
                     optional=[(X, Q.ADVISOR, wk.DIR_OUT, Y),
                               (Y, Q.TYPE_ID, wk.DIR_OUT, Q.FULLPROF)]),
        "union_opt": Plan([grad], 3, [X, Y, Z], unions=unions, blind=True,
                          optional=[(X, Q.ADVISOR, wk.DIR_OUT, Z)]),
    }


def timed(fn):
    t0 = time.perf_counter()
    n = fn()
    return (time.perf_counter() - t0) * 1e6, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--univ", type=int, default=2560)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    store = wk.Store(wk.lubm_gen(a.univ, seed=42))
    gstore = wk.GpuStore(store, device=0)
    out = {"workload": "LUBM-%d, one MI355X, blind counts, arms alternated "
                       "round by round in one process" % a.univ,
           "reps": a.reps, "shapes": {}}
    for name, plan in plans().items():
        if a.only and name != a.only:
            continue
        eng = wk.Engine(gstore)
        gid = eng.graph_build(plan)

        def host():
            os.environ["WK_DEV_GROUPS"] = "0"
            try:
                return eng.run_query_count(plan)
            finally:
                os.environ.pop("WK_DEV_GROUPS", None)

        arms = {"host": host, "dev": lambda: eng.run_query_count(plan),
                "graph": lambda: eng.graph_run(gid)}
        t = {k: [] for k in arms}
        rows = {}
        for r in range(a.warmup + a.reps):
            for k, fn in arms.items():
                us, n = timed(fn)
                rows.setdefault(k, n)
                assert rows[k] == n == rows["host"], (name, k, n, rows)
                if r >= a.warmup:
                    t[k].append(us)
        out["shapes"][name] = {
            "rows": rows["host"],
            **{k: {"median_us": round(statistics.median(v), 1),
                   "min_us": round(min(v), 1), "max_us": round(max(v), 1)}
               for k, v in t.items()}}
        del eng
    print(json.dumps(out))


if __name__ == "__main__":
    main()
