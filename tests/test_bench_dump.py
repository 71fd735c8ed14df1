"""bench.py --dump-outputs helpers (CPU-only: no engine involved)."""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _bench():
    spec = importlib.util.spec_from_file_location(
        "wk_bench", os.path.join(HERE, "..", "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_canonical_table_is_order_independent():
    bench = _bench()
    rng = np.random.default_rng(0)
    tbl = rng.integers(0, 2**32, size=(1000, 3), dtype=np.uint64).astype(np.uint32)
    a = bench.canonical_table(tbl, 1 << 20)
    b = bench.canonical_table(tbl[rng.permutation(len(tbl))], 1 << 20)
    assert a.dtype == np.float64 and a.shape == tbl.shape
    assert np.array_equal(a, b)
    assert np.array_equal(a.astype(np.uint32), tbl[np.lexsort(tbl.T[::-1])])


def test_canonical_table_sample_is_fixed_and_bounded():
    bench = _bench()
    rng = np.random.default_rng(1)
    tbl = rng.integers(0, 2**32, size=(5000, 2), dtype=np.uint64).astype(np.uint32)
    budget = 100 * 2 * 8  # room for 100 rows
    a = bench.canonical_table(tbl, budget)
    b = bench.canonical_table(tbl[::-1], budget)
    assert a.shape == (100, 2) and a.nbytes <= budget
    assert np.array_equal(a, b)
    assert bench.canonical_table(np.empty((0, 4), np.uint32), budget).shape == (0, 4)


def test_dump_outputs_writes_named_arrays(tmp_path):
    bench = _bench()
    tables = {"qa": np.array([[3, 1], [1, 2]], np.uint32),
              "qb": np.empty((0, 1), np.uint32)}
    out = tmp_path / "dump"
    bench.dump_outputs(str(out), ["qa", "qb"], tables["qb"], 0,
                       lambda n: (tables[n].shape[0], tables[n]))
    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    # the empty qb result leaves no (empty) table file, only its zero counts
    assert set(got) == {"last_step_qb_rows", "qa_table", "row_counts"}
    assert all(v.size for v in got.values())
    assert all(v.dtype == np.float64 for v in got.values())
    assert np.array_equal(got["row_counts"], [2.0, 0.0])
    assert np.array_equal(got["qa_table"], [[1.0, 2.0], [3.0, 1.0]])
