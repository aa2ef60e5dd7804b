"""bench.py --dump-outputs without a GPU: what the last step returned, as float64 arrays, the same from run to run, within the size limit,
no array empty."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _csc(rng, ncols, nnz):
    colptr = np.concatenate([[0], np.sort(rng.integers(0, nnz, ncols - 1)), [nnz, nnz]]).astype(np.uint32)   # (the last column empty)
    return colptr, rng.integers(0, 30000, nnz).astype(np.uint32), rng.integers(1, 300, nnz).astype(np.uint32)


class _Ctx:
    """What dump_outputs asks of the context: the number of cells (for merge_targets())."""
    def total_cells_number(self):
        return 1000


def _step_output(seed):
    rng = np.random.default_rng(seed)
    cm, raw = _csc(rng, 400, bench.DUMP_SAMPLE + 12345), _csc(rng, 900, 5000)
    return cm, raw, np.arange(7, 407, dtype=np.uint64), (np.array([3, 9], np.uint64), np.array([1, 2], np.uint64))


def test_dump_outputs_are_the_step_outputs_in_float64(tmp_path):
    out = _step_output(1)
    bench.dump_outputs(str(tmp_path / "a"), out, False, _Ctx())
    bench.dump_outputs(str(tmp_path / "b"), _step_output(1), False, _Ctx())
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"cm_colptr.npy", "cm_raw_sample_value.npy", "filtered_cells.npy", "merge_targets_sample_value.npy"} <= set(names)
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float64 and a.size and np.array_equal(a, b), n
        total += a.nbytes
    assert total <= 64 << 20
    ld = lambda n: np.load(tmp_path / "a" / (n + ".npy"))    # noqa: E731
    for name, (colptr, rows, vals) in (("cm", out[0]), ("cm_raw", out[1])):
        at = ld(name + "_sample_index").astype(np.int64)
        assert len(at) == min(len(rows), bench.DUMP_SAMPLE) and np.all(np.diff(at) > 0)
        col = ld(name + "_sample_col").astype(np.int64)
        assert np.all((colptr[col] <= at) & (at < colptr[col + 1]))
        assert np.array_equal(ld(name + "_sample_row"), rows[at]) and np.array_equal(ld(name + "_sample_value"), vals[at])
        assert np.array_equal(ld(name + "_colptr"), colptr)
        sums = [int(vals[colptr[j]:colptr[j + 1]].sum()) for j in range(len(colptr) - 1)]
        assert ld(name + "_col_sum").tolist() == sums
    assert np.array_equal(ld("filtered_cells"), out[2])
    targets = np.arange(1000)
    targets[[3, 9]] = [1, 2]
    assert np.array_equal(ld("merge_targets_sample_index"), np.arange(1000)) and np.array_equal(ld("merge_targets_sample_value"), targets)


def test_dump_outputs_without_merges_writes_no_empty_array(tmp_path):
    """No CB merge (the default C2 workload): merge_targets() is every cell's own id, and nothing written is empty."""
    cm, raw, cells, _ = _step_output(2)
    bench.dump_outputs(str(tmp_path), (cm, raw, cells, (np.zeros(0, np.uint64), np.zeros(0, np.uint64))), False, _Ctx())
    assert all(np.load(tmp_path / n).size for n in os.listdir(tmp_path))
    assert np.array_equal(np.load(tmp_path / "merge_targets_sample_value.npy"), np.arange(1000))


def test_dump_outputs_of_many_cells_stay_a_bounded_sample(tmp_path):
    """merge_targets() has one entry per cell (millions at C2): a seeded sample of them, the cells' own ids beside their targets."""
    class Many(_Ctx):
        def total_cells_number(self):
            return 5_000_000
    cm, raw, cells, _ = _step_output(3)
    bench.dump_outputs(str(tmp_path), (cm, raw, cells, (np.array([4_999_999], np.uint64), np.array([17], np.uint64))), False, Many())
    at, tgt = np.load(tmp_path / "merge_targets_sample_index.npy"), np.load(tmp_path / "merge_targets_sample_value.npy")
    assert len(at) == bench.DUMP_SAMPLE and np.all(np.diff(at) > 0) and at[-1] < 5_000_000
    assert np.array_equal(tgt, np.where(at == 4_999_999, 17, at))
