"""Plans and plain expectations for the tests of UNION / OPTIONAL groups on
the asynchronous path (a helper module, not a test).

Everything runs on `group_graph.group_graph()`.  The expectations restate
the operators in numpy over the plain adjacency (`synth_graph.step_ref`,
`group_graph.optional_ref`, `filter_ref.keep_mask`) and share no code
with the engine or the oracle: a UNION is the concatenation of the plain
queries `main + branch`, an OPTIONAL is `optional_ref` over the table in
front of it.  `test_group_async_cpu.py` checks every one of them against
the oracle; `test_gpu_group_async.py` holds the engine to them.
"""
import numpy as np

from wukong_amd import Plan
from tests import filter_ref
from tests import group_graph as gg
from tests.group_graph import (BLANK, GT_B, GT_O, P_LIST, P_NOSEG, P_OPT,
                               P_OPT2, P_PAIR, P_TAG, START_SIZES, T_ALL,
                               T_NONE, T_START, TG_A, optional_ref)
from tests.oracle_util import OracleCtx, sort_rows
from tests.synth_graph import IN, OUT, TYPE, step_ref

X, Y, Z, W, V = -1, -2, -3, -4, -5
SETS = [T_START[n] for n in START_SIZES] + [T_NONE, T_ALL]
PARENTS = [T_START[n] for n in START_SIZES]
_NONE = np.empty(0, dtype=np.uint32)


def bgp_ref(adj, pats):
    """A plain BGP that opens with an index start, one operator after the
    other; (table, {variable: column}), columns in binding order."""
    table, v2c = None, {}
    for s, p, d, o in pats:
        if table is None:
            assert s >= 0 and p == TYPE and d == IN and o < 0
            table = adj.get((s, TYPE, IN), _NONE)[:, None]
            v2c[o] = 0
        elif s >= 0:                              # const_to_known
            keep = np.isin(table[:, v2c[o]], adj.get((s, p, d), _NONE))
            table = table[keep]
        elif o >= 0:
            table = step_ref(table, v2c[s], adj, "k2c", p, d, const=o)
        elif o in v2c:
            table = step_ref(table, v2c[s], adj, "k2k", p, d, col2=v2c[o])
        else:
            table = step_ref(table, v2c[s], adj, "k2u", p, d)
            v2c[o] = table.shape[1] - 1
    return table, v2c


class Cases:
    """The graph, its adjacency, the oracle and memoised expectations."""

    def __init__(self):
        self.triples, self.meta = gg.group_graph()
        self.adj = gg.group_adjacency(self.triples)
        self._ora = None
        self._ref = {}

    @property
    def ora(self):
        if self._ora is None:
            self._ora = OracleCtx(self.triples)
        return self._ora

    def memo(self, key, fn):
        if key not in self._ref:
            r = sort_rows(fn())
            r.setflags(write=False)
            self._ref[key] = r
        return self._ref[key]

    def members(self, t):
        return self.adj.get((t, TYPE, IN), _NONE)

    # ---- UNION --------------------------------------------------------
    def union_shapes(self):
        """name -> (main patterns after the index start, branches, nvars).
        Every branch of a shape binds the same variables in the same
        order, which is the layout the engine requires."""
        c = int(self.meta["c_list"])
        tag0 = int(self.meta["tv"][0])
        return {
            # the parent is a zero-copy view of the index list
            "view-2": ([], [[(X, P_TAG, OUT, Y)], [(X, P_PAIR, OUT, Y)]], 2),
            # 1 column: filters only (k2c, const_to_known)
            "view-1col": ([], [[(X, P_TAG, OUT, tag0)],
                               [(c, P_LIST, OUT, X)]], 1),
            # an owned 2-column parent; the first branch has two patterns
            # (expansion, then a filter that drops rows) and its ping-pong
            # overwrites the parent's buffer; the second one is empty (no
            # segment of that predicate)
            "owned-3": ([(X, P_TAG, OUT, Z)],
                        [[(X, P_OPT, OUT, Y), (Y, TYPE, OUT, GT_B)],
                         [(X, P_NOSEG, OUT, Y)],
                         [(X, P_PAIR, OUT, Y)]], 3),
            "owned-2": ([(X, P_TAG, OUT, Z)],
                        [[(X, P_PAIR, OUT, Y), (Y, TYPE, OUT, GT_O)],
                         [(X, P_OPT, OUT, Y)]], 3),
            # 5 columns
            "wide": ([(X, P_TAG, OUT, Y), (X, P_PAIR, OUT, Z)],
                     [[(X, P_TAG, OUT, W), (Z, P_OPT2, OUT, V)],
                      [(X, P_NOSEG, OUT, W), (Z, P_OPT2, OUT, V)],
                      [(X, P_TAG, OUT, W), (Z, P_OPT2, OUT, V),
                       (V, TYPE, OUT, GT_B)]], 5),
            # the main BGP yields no row
            "empty": ([(X, TYPE, OUT, TG_A)],
                      [[(X, P_TAG, OUT, Y)], [(X, P_PAIR, OUT, Y)]], 2),
        }

    def union_parents(self, shape):
        if shape == "wide":
            return [T_START[1], T_START[255], T_START[257]]
        if shape == "empty":
            return [T_START[257]]
        return PARENTS

    def union_main(self, shape, t):
        return [(t, TYPE, IN, X)] + self.union_shapes()[shape][0]

    def union_plan(self, shape, t, **kw):
        main, branches, nv = self.union_shapes()[shape]
        return Plan([(t, TYPE, IN, X)] + main, nv,
                    [-(k + 1) for k in range(nv)], unions=branches, **kw)

    def branch_plans(self, shape, t):
        """The plain query of every branch: main + branch."""
        main, branches, nv = self.union_shapes()[shape]
        return [Plan([(t, TYPE, IN, X)] + main + list(b), nv,
                     [-(k + 1) for k in range(nv)]) for b in branches]

    def branch_tables(self, shape, t):
        """Unsorted per-branch tables, columns in variable order."""
        _, branches, nv = self.union_shapes()[shape]
        out = []
        for b in branches:
            tbl, v2c = bgp_ref(self.adj, self.union_main(shape, t) + list(b))
            out.append(tbl[:, [v2c[-(k + 1)] for k in range(nv)]])
        return out

    def union_want(self, shape, t):
        return self.memo(("union", shape, t),
                         lambda: np.vstack(self.branch_tables(shape, t)))

    # ---- OPTIONAL (the groups of test_gpu_group_edges.py, restated) ----
    def opt_groups(self):
        c = int(self.meta["c_list"])
        return {
            "k2u": [(X, P_OPT, OUT, Y)],
            "k2u-type": [(X, P_OPT, OUT, Y), (Y, TYPE, OUT, GT_B)],
            "k2u-k2u-type": [(X, P_OPT, OUT, Y), (Y, P_OPT2, OUT, Z),
                             (Z, TYPE, OUT, GT_B)],
            "k2u-type-k2u": [(X, P_OPT, OUT, Y), (Y, TYPE, OUT, GT_B),
                             (Y, P_OPT2, OUT, Z)],
            "c2k": [(X, P_OPT, OUT, Y), (c, P_LIST, OUT, Y)],
            "c2k-k2u": [(c, P_LIST, OUT, X), (X, P_OPT, OUT, Y)],
            "k2k": [(X, P_OPT, OUT, Y), (X, P_PAIR, OUT, Y)],
            "index": [(X, P_TAG, OUT, Y), (Y, TYPE, OUT, Z), (Z, TYPE, IN, W)],
        }

    def opt_plan(self, group, t, **kw):
        pats = self.opt_groups()[group]
        nv = -min(min(s, o) for s, p, d, o in pats)
        return Plan([(t, TYPE, IN, X)], nv, [-(k + 1) for k in range(nv)],
                    optional=pats, **kw)

    def opt_want(self, group, t):
        return self.memo(("opt", group, t), lambda: optional_ref(
            self.members(t)[:, None], self.opt_groups()[group], self.adj))

    # an owned (expanded) parent in front of a two-pattern group
    def opt_owned_plan(self, t):
        return Plan([(t, TYPE, IN, X), (X, P_TAG, OUT, Y)], 4, [X, Y, Z, W],
                    optional=[(X, P_OPT, OUT, Z), (Z, P_OPT2, OUT, W)])

    def opt_owned_want(self, t):
        def fn():
            base, _ = bgp_ref(self.adj, [(t, TYPE, IN, X), (X, P_TAG, OUT, Y)])
            return optional_ref(base, [(X, P_OPT, OUT, Z),
                                       (Z, P_OPT2, OUT, W)], self.adj)
        return self.memo(("opt-owned", t), fn)

    # ---- UNION, then OPTIONAL, then a FILTER on a group-born variable ----
    COMBO_T = T_START[257]
    COMBO_UNIONS = [[(X, P_TAG, OUT, Y)], [(X, P_PAIR, OUT, Y)]]
    COMBO_OPT = [(Y, P_OPT2, OUT, Z)]

    def combo_filters(self):
        zc = int(self.meta["zpool"][5])
        return {
            "none": [],
            "bound": [("bound", Z)],
            "not-bound": [("not", ("bound", Z))],
            # BLANK is an ordinary value: `=` fails on it, `!=` holds
            "eq-const": [("eq", Z, zc)],
            "ne-const": [("ne", Z, zc)],
            "or": [("or", ("eq", Z, zc), ("not", ("bound", Z)))],
        }

    def combo_plan(self, fname, **kw):
        return Plan([(self.COMBO_T, TYPE, IN, X)], 3, [X, Y, Z],
                    unions=self.COMBO_UNIONS, optional=self.COMBO_OPT,
                    filters=self.combo_filters()[fname], **kw)

    def combo_want(self, fname):
        def full():
            base = self.members(self.COMBO_T)[:, None]
            u = np.vstack([step_ref(base, 0, self.adj, "k2u", P_TAG, OUT),
                           step_ref(base, 0, self.adj, "k2u", P_PAIR, OUT)])
            return optional_ref(u, self.COMBO_OPT, self.adj)

        def fn():
            tbl = np.array(self.memo(("combo", "none"), full))
            return tbl[filter_ref.keep_mask(tbl, self.combo_filters()[fname])]
        return self.memo(("combo", fname), fn if fname != "none" else full)

    # ---- a plain plan, for suites and buffer identity ------------------
    PLAIN = Plan([(T_START[513], TYPE, IN, X), (X, P_PAIR, OUT, Y)], 2, [X, Y])

    def plain_want(self):
        return self.memo("plain", lambda: bgp_ref(
            self.adj, self.PLAIN.patterns)[0])


def same(got, want):
    """Shapes equal and rows equal after sorting (`want` is sorted)."""
    got = np.asarray(got)
    return got.shape == want.shape and np.array_equal(sort_rows(got), want)
