"""bench.py --dump-outputs: which rows are written and how (the GPU side, a plain run that dumps its
last step, is in test_gpu_multirank.py with the other runs of the benchmark)."""
import os

import numpy as np


def dumped_words(path, name="pbs_out"):
    hi = np.load(os.path.join(path, name + "_hi32.npy"))
    lo = np.load(os.path.join(path, name + "_lo32.npy"))
    assert hi.dtype == np.float64 and lo.dtype == np.float64
    return (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)


def test_dump_rows_fixed_sample_within_budget():
    import bench
    # the metric's batch: a sample, the same one on every call, sorted and without repeats
    rows = bench.dump_rows(4096, 2049)
    assert np.array_equal(rows, bench.dump_rows(4096, 2049))
    assert len(rows) == bench.DUMP_MAX_ROWS and len(set(rows.tolist())) == len(rows)
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < 4096
    # a small batch is written whole
    assert np.array_equal(bench.dump_rows(96, 2049), np.arange(96))
    # every shape stays under 64 MB in all: long rows (N = 65536) and eight ranks
    for batch, words, world in ((4096, 2049, 1), (512, 65537, 1), (8192, 2049, 8), (1, 65537, 1)):
        n = len(bench.dump_rows(batch, words, world))
        assert 1 <= n <= batch and world * n * words * 16 + world * n * 8 <= 64_000_000


def test_dump_outputs_round_trip_exact(tmp_path):
    import bench
    rng = np.random.RandomState(7)
    words = rng.randint(0, 1 << 62, size=(5, 33)).astype(np.uint64) * np.uint64(4) + np.uint64(3)
    words[0, 0], words[0, 1] = np.uint64(0), np.uint64(0xFFFFFFFFFFFFFFFF)
    rows = np.array([1, 4, 6, 7, 9])
    bench.dump_outputs(str(tmp_path / "d"), words, rows)
    assert np.array_equal(dumped_words(str(tmp_path / "d")), words)
    assert np.array_equal(np.load(tmp_path / "d" / "pbs_out_rows.npy"), rows.astype(np.float64))
    bench.dump_outputs(str(tmp_path / "d"), words, rows, rank=1, world=2)
    assert np.array_equal(dumped_words(str(tmp_path / "d"), "pbs_out_rank1"), words)
