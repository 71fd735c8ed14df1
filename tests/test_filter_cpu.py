"""FILTER (=, !=, bound, &&, ||, !) above the GPU: parser, Plan encoding
and validation, the planner pass-through, the reference evaluator and
the distributed driver (world 2, gloo, oracle executors).

Expected results come from tests/filter_ref.py over the oracle's table
of the same plan without the filter; every comparison is exact.  Each
data-dependent case asserts that the filter keeps some rows and drops
some, so none passes vacuously.
"""
import os

import numpy as np
import pytest
import torch.multiprocessing as mp

import wukong_amd as wk
from wukong_amd import Plan, planner, sparql
from wukong_amd import queries as Q
from tests import filter_ref
from tests.oracle_util import OracleCtx, sort_rows

BLANK = filter_ref.BLANK
HEAD = "PREFIX ub: <http://swat/onto/> PREFIX rdf: <http://w3/rdf/> "
X, Y, Z = -1, -2, -3


def _parse(where, sel="?x ?y"):
    return sparql.parse(HEAD + "SELECT %s WHERE { %s }" % (sel, where),
                        sparql.lubm_vocab())


# variables get their ids in order of first use: ?x -1, ?y -2, ?z -3
ADV = "?x ub:advisor ?y . ?z ub:advisor ?y . "


# ---------------------------------------------------------------------
# parser
# ---------------------------------------------------------------------
@pytest.mark.parametrize("text,want", [
    ("?x = ?y", ("eq", X, Y)),
    ("?x != ?y", ("ne", X, Y)),
    ("bound(?z)", ("bound", Z)),
    ("BOUND ( ?z )", ("bound", Z)),
    ("!bound(?z)", ("not", ("bound", Z))),
    ("?x = ?y && ?y != ?z", ("and", ("eq", X, Y), ("ne", Y, Z))),
    ("?x = ?y || ?y != ?z", ("or", ("eq", X, Y), ("ne", Y, Z))),
    # && binds tighter than ||
    ("?x = ?y || ?y = ?z && ?x != ?z",
     ("or", ("eq", X, Y), ("and", ("eq", Y, Z), ("ne", X, Z)))),
    ("(?x = ?y || ?y = ?z) && ?x != ?z",
     ("and", ("or", ("eq", X, Y), ("eq", Y, Z)), ("ne", X, Z))),
    ("?x = ?y || ?y = ?z || ?x = ?z",
     ("or", ("or", ("eq", X, Y), ("eq", Y, Z)), ("eq", X, Z))),
    ("!(!(?x = ?y))", ("not", ("not", ("eq", X, Y)))),
    ("!!!bound(?x)", ("not", ("not", ("not", ("bound", X))))),
    ("!(?x = ?y && !(bound(?z) || ?z != ?x))",
     ("not", ("and", ("eq", X, Y),
              ("not", ("or", ("bound", Z), ("ne", Z, X)))))),
    # constants: any vocabulary-resolved term, on either side
    ("?y = ub:Course", ("eq", Y, Q.COURSE)),
    ("<http://www.University0.edu> != ?x", ("ne", Q.UNIV0, X)),
    ("?x=?y&&?y!=ub:Course", ("and", ("eq", X, Y), ("ne", Y, Q.COURSE))),
])
def test_parse_expression(text, want):
    p = _parse(ADV + "FILTER(%s)" % text)
    assert p.filters == [want]
    assert len(p.patterns) == 2 and p.nvars == 3


def test_parse_placement_and_clauses():
    # ?x -1, ?z -2, ?y -3: the patterns come first, whatever the text order
    want = [("ne", -1, -3), ("bound", -2)]
    for where in (
            "?x ub:advisor ?z . FILTER(?x != ?y) ?y ub:advisor ?z . "
            "FILTER(bound(?z))",
            "?x ub:advisor ?z . FILTER (?x != ?y) . ?y ub:advisor ?z . "
            "filter(bound(?z)) .",
            "?x ub:advisor ?z FILTER(?x != ?y) ?y ub:advisor ?z "
            "FILTER(bound(?z))"):
        p = _parse(where)
        assert p.filters == want, where
        assert p.patterns == [(-1, Q.ADVISOR, 1, -2), (-3, Q.ADVISOR, 1, -2)]
    # .fmt directives still number the triples alone
    p = sparql.parse(HEAD + "SELECT ?x ?y WHERE { ?x ub:advisor ?z . "
                     "FILTER(?x != ?y) ?y ub:advisor ?z }",
                     sparql.lubm_vocab(), plan_lines=["2 >", "1 <"])
    assert p.patterns == [(-1, Q.ADVISOR, 1, -2), (-2, Q.ADVISOR, 0, -3)]
    assert p.filters == [("ne", -3, -1)]
    # a FILTER next to OPTIONAL / UNION groups of the main group
    p = _parse("?x rdf:type ub:GraduateStudent . OPTIONAL { ?x ub:advisor "
               "?y } FILTER(!bound(?y))")
    assert p.filters == [("not", ("bound", Y))] and len(p.optional) == 1
    # a variable used only in the filter still gets an id
    p = _parse(ADV + "FILTER(?w != ?x)")
    assert p.nvars == 4 and p.filters == [("ne", -4, X)]


@pytest.mark.parametrize("where,needle", [
    (ADV + "FILTER(?x < ?y)", "DESIGN §7"),
    (ADV + "FILTER(?x >= ?y)", "DESIGN §7"),
    (ADV + "FILTER(regex(?x, \"a\"))", "DESIGN §7"),
    (ADV + "FILTER(isIRI(?x))", "DESIGN §7"),
    (ADV + "FILTER(isLiteral(?x) && ?x != ?y)", "DESIGN §7"),
    (ADV + "FILTER(?x + ?y = ?z)", "DESIGN §7"),
    (ADV + "FILTER(?x = ub:NoSuchThing)", "unknown vocabulary term"),
    (ADV + "FILTER((?x != ?y)", "unbalanced"),
    (ADV + "FILTER(?x != ?y))", ""),
    (ADV + "FILTER ?x != ?y", "'('"),
    (ADV + "FILTER(?x != )", ""),
    (ADV + "FILTER(bound(ub:Course))", "variable"),
    ("?x rdf:type ub:GraduateStudent . OPTIONAL { ?x ub:advisor ?y . "
     "FILTER(?x != ?y) }", "DESIGN §7"),
    ("?x rdf:type ub:GraduateStudent . { ?x ub:advisor ?y FILTER(?x != ?y) }"
     " UNION { ?x ub:memberOf ?y }", "DESIGN §7"),
])
def test_parse_errors(where, needle):
    with pytest.raises(sparql.ParseError) as ei:
        _parse(where)
    assert needle in str(ei.value)


# ---------------------------------------------------------------------
# Plan: encoding and validation
# ---------------------------------------------------------------------
NAMES = {v[0]: k for k, v in wk.FILTER_OPS.items()}


def decode(cplan):
    """Nested tuples back from a wk_plan_t postfix program (a stack
    machine of its own, not to_c run backwards)."""
    stack = []
    for i in range(cplan.nfilter):
        n = cplan.filter[i]
        name = NAMES[n.op]
        if name in ("eq", "ne"):
            stack.append((name, n.a, n.b))
        elif name == "bound":
            stack.append((name, n.a))
        elif name == "not":
            stack.append((name, stack.pop()))
        else:
            r, l = stack.pop(), stack.pop()
            stack.append((name, l, r))
    assert len(stack) == 1
    return stack[0]


def _and_chain(n):
    """n leaves ANDed left-deep: 2n - 1 nodes."""
    e = ("ne", X, Y)
    for _ in range(n - 1):
        e = ("and", e, ("ne", X, Y))
    return e


def test_to_c_postfix():
    pats = [(7, 1, 0, X), (X, 2, 1, Y), (Y, 3, 1, Z)]
    deep = ("or", ("ne", X, Y), ("not", ("and", ("bound", Z),
                                         ("or", ("eq", 99, Z), ("eq", X, X)))))
    c = Plan(pats, 3, [X], filters=[deep]).to_c()
    assert c.nfilter == 8 and decode(c) == deep
    ops = [NAMES[c.filter[i].op] for i in range(c.nfilter)]
    assert ops == ["ne", "bound", "eq", "eq", "or", "and", "not", "or"]
    # several clauses are ONE program, ANDed left to right
    c = Plan(pats, 3, [X], filters=[("ne", X, Y), ("bound", Z), deep]).to_c()
    assert decode(c) == ("and", ("and", ("ne", X, Y), ("bound", Z)), deep)
    c = Plan(pats, 3, [X]).to_c()
    assert c.nfilter == 0 and not c.filter
    # 16 leaves + 15 ANDs + 1 NOT = 32 nodes: the largest program
    c = Plan(pats, 3, [X], filters=[("not", _and_chain(16))]).to_c()
    assert c.nfilter == 32 and decode(c) == ("not", _and_chain(16))


@pytest.mark.parametrize("flt", [
    [("lt", X, Y)],                       # bad op
    [("regex", X)],
    [(1, X, Y)],
    ["ne"],
    [("ne", X)],                          # bad arity
    [("ne", X, Y, Z)],
    [("bound", X, Y)],
    [("not", ("bound", X), ("bound", Y))],
    [("and", ("bound", X))],
    [("or", ("bound", X), ("bound", Y), ("bound", Z))],
    [("ne", X, -4)],                      # variable out of range
    [("bound", -4)],
    [("not", ("or", ("eq", X, Y), ("eq", -9, Y)))],
    [("eq", X, 0)],                       # neither variable nor constant
    [("bound", 5)],
    [("eq", X, "a")],
    [("not", _and_chain(17))],            # 34 nodes
    [("ne", X, Y)] * 17,                  # 17 leaves + 16 ANDs = 33
])
def test_plan_constructor_errors(flt):
    with pytest.raises(ValueError):
        Plan([(7, 1, 0, X), (X, 2, 1, Y), (Y, 3, 1, Z)], 3, [X], filters=flt)


def test_plan_text_keeps_filters(lubm2):
    store = wk.Store(lubm2)
    text = (HEAD + "SELECT ?x ?y WHERE { ?x ub:advisor ?z . ?y ub:advisor ?z"
            " . ?x rdf:type ub:GraduateStudent . FILTER(?x != ?y) "
            "FILTER(?z != ub:Course || bound(?z)) }")
    p = planner.plan_text(store, text, sparql.lubm_vocab())
    want = [("ne", -1, -3), ("or", ("ne", -2, Q.COURSE), ("bound", -2))]
    assert p.filters == want and len(p.patterns) == 3 and p.nvars == 3
    p2 = planner.plan_patterns(store, p.patterns, 3, [X, Y], filters=want)
    assert p2.filters == want and p2.to_c().nfilter == 5


# ---------------------------------------------------------------------
# the reference evaluator, on hand-written tables
# ---------------------------------------------------------------------
def test_filter_ref_by_hand():
    B_ = BLANK
    t = np.array([[5, 5, 9],
                  [5, 6, 9],
                  [7, B_, B_],
                  [B_, B_, 3]], dtype=np.uint32)

    def m(*f):
        return filter_ref.keep_mask(t, list(f)).tolist()

    assert m(("eq", X, Y)) == [True, False, False, True]   # blank == blank
    assert m(("ne", X, Y)) == [False, True, True, False]
    assert m(("eq", 5, X)) == [True, True, False, False]
    assert m(("ne", Z, 9)) == [False, False, True, True]   # unbound != c
    assert m(("bound", Y)) == [True, True, False, False]
    assert m(("not", ("bound", Y))) == [False, False, True, True]
    assert m(("and", ("bound", Z), ("not", ("bound", X)))) == \
        [False, False, False, True]
    assert m(("or", ("eq", X, Y), ("eq", Y, 6))) == [True, True, False, True]
    assert m(("eq", X, Y), ("bound", X)) == [True, False, False, False]
    assert m() == [True] * 4
    assert filter_ref.keep_mask(t[:0], [("eq", X, Y)]).tolist() == []
    with pytest.raises(AssertionError):
        m(("xor", X, Y))


# ---------------------------------------------------------------------
# distributed driver, world 2 (gloo), oracle executors
# ---------------------------------------------------------------------
def _dist_plans():
    g = (Q.GRADSTUDENT, Q.TYPE_ID, wk.DIR_IN, X)
    return {
        # grad students of department 0 or with a degree from university 0
        "plain": Plan([g, (X, Q.MEMBEROF, wk.DIR_OUT, Y),
                       (X, Q.UGDEGREE, wk.DIR_OUT, Z)], 3, [X, Y, Z],
                      filters=[("or", ("eq", Y, Q.DEPT0_UNIV0),
                                ("eq", Q.UNIV0, Z))]),
        # two students of the same advisor, DISTINCT/LIMIT after the filter
        # (variable ids in column order: DISTINCT sorts whole rows)
        "pairs": Plan([(Q.DEPT0_UNIV0, Q.MEMBEROF, wk.DIR_IN, X),
                       (X, Q.ADVISOR, wk.DIR_OUT, Y),
                       (Y, Q.ADVISOR, wk.DIR_IN, Z)], 3, [X, Z],
                      distinct=True, limit=40, offset=3,
                      filters=[("ne", X, Z)]),
        # branch-born variable
        "union": Plan([g], 2, [X, Y],
                      unions=[[(X, Q.MEMBEROF, wk.DIR_OUT, Y)],
                              [(X, Q.UGDEGREE, wk.DIR_OUT, Y)]],
                      filters=[("or", ("eq", Y, Q.UNIV0),
                                ("eq", Y, Q.DEPT0_UNIV0))]),
        # the OPTIONAL negation idiom and its complement
        "opt-unbound": Plan([(Q.UGSTUDENT, Q.TYPE_ID, wk.DIR_IN, X)], 2,
                            [X, Y], optional=[(X, Q.ADVISOR, wk.DIR_OUT, Y)],
                            filters=[("not", ("bound", Y))]),
        "opt-bound": Plan([(Q.UGSTUDENT, Q.TYPE_ID, wk.DIR_IN, X),
                           (X, Q.MEMBEROF, wk.DIR_OUT, Z)], 3, [X, Y, Z],
                          optional=[(X, Q.ADVISOR, wk.DIR_OUT, Y)],
                          filters=[("bound", Y), ("ne", Z, Q.DEPT0_UNIV0)]),
    }


def _worker(rank, world, port, results):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch.distributed as dist
    from wukong_amd.dist import DistQuery
    from tests.oracle_util import OracleExecutor

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ctx = OracleCtx(wk.lubm_gen(2, seed=42, sid=rank, nsrv=world),
                        sid=rank, nsrv=world)
        out = {}
        for name, plan in _dist_plans().items():
            dq = DistQuery(OracleExecutor(ctx, plan), plan, rank, world,
                           threshold=0)
            dq.run()
            out[name] = sort_rows(dq.gather_result())
        if rank == 0:
            results.put(out)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_dist_filters_two_ranks_equal_single():
    ctx = mp.get_context("spawn")
    results = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, 29884, results))
             for r in range(2)]
    for p in procs:
        p.start()
    got = results.get(timeout=240)
    for p in procs:
        p.join(timeout=60)
    full = OracleCtx(wk.lubm_gen(2, seed=42))
    for name, plan in _dist_plans().items():
        st = {}
        want = filter_ref.expected(full, plan, st)
        assert 0 < st["after"] < st["before"], (name, st)
        if plan.limit < 0:
            want = sort_rows(want)
            assert got[name].shape == want.shape, (name, got[name].shape)
            assert np.array_equal(got[name], want), name
        else:
            # DISTINCT + OFFSET/LIMIT cut a sorted table: same rows
            assert np.array_equal(got[name], sort_rows(want)), name
