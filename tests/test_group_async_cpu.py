"""The expectations of test_gpu_group_async.py are right: every plain-numpy
expectation of tests/group_async_cases.py equals the oracle's result of
the same plan on the same triples.  A UNION expectation is the
concatenation of the per-branch plain queries, an OPTIONAL one is
`group_graph.optional_ref`.  No GPU."""
import numpy as np
import pytest

from tests import filter_ref
from tests.group_async_cases import Cases, SETS, same
from tests.group_graph import BLANK, START_SIZES, T_START
from tests.oracle_util import sort_rows


@pytest.fixture(scope="module")
def cx():
    return Cases()


def test_union_expectations(cx):
    for shape in cx.union_shapes():
        for t in cx.union_parents(shape):
            want = cx.union_want(shape, t)
            assert same(cx.ora.run_query(cx.union_plan(shape, t)), want), \
                (shape, t)
            # ... and the oracle's own per-branch plain queries, stacked
            parts = [cx.ora.run_query(p) for p in cx.branch_plans(shape, t)]
            nv = cx.union_shapes()[shape][2]
            stacked = np.vstack([np.asarray(p).reshape(-1, nv) for p in parts])
            assert same(stacked, want), (shape, t)


def test_union_cases_are_not_vacuous(cx):
    sizes = {}
    for shape in cx.union_shapes():
        nv = cx.union_shapes()[shape][2]
        for t in cx.union_parents(shape):
            parts = cx.branch_tables(shape, t)
            n = [len(p) for p in parts]
            sizes[(shape, t)] = n
            assert cx.union_want(shape, t).shape == (sum(n), nv)
    big = T_START[1025]
    # both branches contribute; the P_NOSEG branch is empty; the filter
    # branch keeps some rows and drops others
    assert all(sizes[("view-2", big)])
    a, b, c = sizes[("owned-3", big)]
    assert a > 0 and b == 0 and c > 0
    assert a < len(cx.opt_want("k2u", big))
    assert sizes[("empty", T_START[257])] == [0, 0]
    assert all(sizes[("view-1col", big)])
    # word counts of the copies on both sides of a multiple of 4: the
    # 16-byte body with and without a scalar tail
    words = {sum(n) * cx.union_shapes()[s][2] % 4 for (s, t), n in sizes.items()}
    assert len(words) >= 3, words
    w = cx.union_want("wide", T_START[257])
    assert w.shape[1] == 5 and len(w) > 256


def test_optional_expectations(cx):
    for group in cx.opt_groups():
        for t in SETS:
            want = cx.opt_want(group, t)
            assert same(cx.ora.run_query(cx.opt_plan(group, t)), want), \
                (group, t)
    for n in (257, 1025):
        t = T_START[n]
        want = cx.opt_owned_want(t)
        assert same(cx.ora.run_query(cx.opt_owned_plan(t)), want), n
        assert (want[:, 2] == BLANK).any() and (want[:, 3] != BLANK).any()


def test_combination_expectations(cx):
    full = cx.combo_want("none")
    assert same(cx.ora.run_query(cx.combo_plan("none")), full)
    for name in cx.combo_filters():
        want = cx.combo_want(name)
        got = filter_ref.expected(cx.ora, cx.combo_plan(name))
        assert same(got, want), name
        if name != "none":
            assert 0 < len(want) < len(full), name
    assert len(cx.combo_want("bound")) + len(cx.combo_want("not-bound")) == \
        len(full)
    assert len(cx.combo_want("or")) == \
        len(cx.combo_want("eq-const")) + len(cx.combo_want("not-bound"))


def test_plain_expectation_and_overflow_counts(cx):
    assert same(cx.ora.run_query(cx.PLAIN), cx.plain_want())
    # the counts the overflow tests size their capacity from
    a, b = [len(p) for p in cx.branch_tables("view-2", T_START[1025])]
    assert a == 1025 and b > a
    assert len(cx.opt_want("k2u", T_START[1025])) > 4 * 1025
    assert sorted(START_SIZES) == START_SIZES
    assert np.array_equal(sort_rows(cx.plain_want()), cx.plain_want())
