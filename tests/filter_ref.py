"""Reference evaluator for FILTER expressions (a helper module, not a
test).

The oracle has no FILTER, so the expected result of a filtered plan is
this evaluator applied to the oracle's full table of the same plan
WITHOUT the filter (every variable projected, no final ops), followed by
`dist.final_process`.  It walks the nested-tuple form row by row in
plain Python and shares no code with `Plan.to_c`, the kernel or the
numpy evaluator of `wukong_amd.dist`.

Semantics: ids compare verbatim, BLANK_ID is an ordinary
value (`?x = ?y` with both unbound is true), `bound(?x)` is
`x != BLANK_ID`, `!` is plain negation, the clauses of a list are ANDed.
"""
import numpy as np

import wukong_amd as wk
from wukong_amd import dist

BLANK = 0xFFFFFFFF


def holds(expr, row):
    """Truth value of one expression on one row (a sequence indexed by
    variable: row[k] is the value of variable -(k + 1))."""
    head = expr[0]

    def val(x):
        return int(row[-x - 1]) if x < 0 else int(x)

    if head == "eq":
        return val(expr[1]) == val(expr[2])
    if head == "ne":
        return val(expr[1]) != val(expr[2])
    if head == "bound":
        return val(expr[1]) != BLANK
    if head == "not":
        return not holds(expr[1], row)
    if head == "and":
        return holds(expr[1], row) and holds(expr[2], row)
    if head == "or":
        return holds(expr[1], row) or holds(expr[2], row)
    raise AssertionError("unknown op %r" % (head,))


def keep_mask(table, filters):
    """Bool mask over the rows of `table`, whose column k holds variable
    -(k + 1)."""
    return np.array([all(holds(f, r) for f in filters)
                     for r in np.asarray(table).tolist()], dtype=bool)


def unfiltered(plan):
    """The same plan without filter and final ops, every variable
    projected in id order (column k = variable -(k + 1))."""
    return wk.Plan(plan.patterns, plan.nvars,
                   [-(k + 1) for k in range(plan.nvars)],
                   optional=plan.optional, unions=plan.unions)


def expected(ora, plan, stats=None):
    """Expected result of `plan` (with filters): oracle table of the
    unfiltered plan -> keep_mask -> final ops.  `stats`, a dict, receives
    the row counts before and after the filter."""
    full = np.asarray(ora.run_query(unfiltered(plan)))
    full = full.reshape(-1, plan.nvars)
    kept = full[keep_mask(full, plan.filters)] if len(full) else full
    if stats is not None:
        stats["before"], stats["after"] = len(full), len(kept)
    return dist.final_process(kept, list(range(plan.nvars)), plan)
