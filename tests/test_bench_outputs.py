"""bench.py --dump-outputs and the plain run's result line.

CPU: dump_outputs on a synthetic result (sample placement, bit order, coverage, formats).
GPU: one short plain run of bench.py: --steps sets the timed steps, the legs behind --full are
null, and the dumped arrays are the run's results (island count, score count, path totals)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from cpgisland_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"estep", "labelled_counts", "scores", "islands", "path_sample", "path_blocks",
         "path_popcount"}


def _load(d):
    out = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
    assert set(out) == NAMES
    assert all(v.dtype in (np.float32, np.float64) for v in out.values())
    assert sum(v.nbytes for v in out.values()) <= 64 << 20
    return out


# sizes: every base sampled, with a ragged last byte / sampled blocks, with a ragged last word
@pytest.mark.parametrize("n", [3 * bench.DUMP_BLOCK + 13, 70 * bench.DUMP_BLOCK + 41])
def test_dump_outputs_arrays(tmp_path, n):
    rng = np.random.default_rng(n)
    words = rng.integers(0, 1 << 32, (n + 31) // 32, dtype=np.uint32)
    bits = ((words[:, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(np.uint8).ravel()[:n]
    isl = np.zeros(5, _lib.ISLAND_DTYPE)
    isl["beg1"], isl["end1"], isl["cg"] = np.arange(5) + 1, np.arange(5) + 300, 0.625
    est, cnt = rng.random(105), rng.integers(0, 1 << 40, 124)
    sc = -rng.random(n >> 20)
    for d in ("a", "b"):   # (twice: the sampled blocks are the same in every run)
        bench.dump_outputs(str(tmp_path / d), est, cnt, words.view(np.int32), sc, isl, n)
    o, o2 = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert all(np.array_equal(o[k], o2[k]) for k in NAMES)
    assert np.array_equal(o["estep"], est) and np.array_equal(o["labelled_counts"], cnt)
    assert np.array_equal(o["scores"], sc)
    assert o["islands"].shape == (5, len(_lib.ISLAND_DTYPE.names))
    assert np.array_equal(o["islands"][:, 1], isl["end1"]) and np.all(o["islands"][:, 4] == 0.625)
    starts = o["path_blocks"].astype(np.int64)
    if n // bench.DUMP_BLOCK <= bench.DUMP_BLOCKS:
        assert np.array_equal(starts, [0]) and np.array_equal(o["path_sample"], bits)
    else:
        assert len(starts) == bench.DUMP_BLOCKS and np.all(np.diff(starts) > 0)
        assert np.all(starts % bench.DUMP_BLOCK == 0) and starts[-1] + bench.DUMP_BLOCK <= n
        assert np.array_equal(o["path_sample"], np.concatenate(
            [bits[s:s + bench.DUMP_BLOCK] for s in starts]))
    pad = np.concatenate([bits, np.zeros(-n % bench.DUMP_POP, np.uint8)])
    assert np.array_equal(o["path_popcount"], pad.reshape(-1, bench.DUMP_POP).sum(1))


def test_dump_outputs_no_islands(tmp_path):
    bench.dump_outputs(str(tmp_path), np.zeros(105), np.zeros(124, np.int64),
                       np.zeros(4, np.int32), np.zeros(0), np.zeros(0, _lib.ISLAND_DTYPE), 100)
    assert _load(tmp_path)["islands"].shape == (0, len(_lib.ISLAND_DTYPE.names))


@pytest.mark.gpu
def test_bench_plain_run_line_and_dump(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n = 5 * (1 << 20) + 4321   # 5 whole decode chunks + a tail the decode leaves out
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
                        "--warmup", "1", "--settle-ms", "0", "--bases", str(n),
                        "--dump-outputs", str(tmp_path / "d")],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["metric"] == bench.METRIC and d["unit"] == "bases/s" and d["dtype"] == "f64"
    assert d["higher_is_better"] is True
    assert d["steps"] == 3 and d["warmup_steps_run"] == 1
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(n / (d["ms_per_step"] / 1e3), rel=1e-9)
    for k in ("cpu_baseline", "fingerprint", "bw_iteration", "cold_cache", "c3_single_gpu"):
        assert d[k] is None
    o = _load(tmp_path / "d")
    assert o["islands"].shape[0] == d["config"]["islands_found"]
    assert o["scores"].shape == (5,) and np.all(o["scores"] < 0)
    assert o["path_sample"].shape == (5 << 20,)   # the decoded chunks, every base (40 blocks)
    assert set(np.unique(o["path_sample"])) <= {0.0, 1.0}
    assert o["path_popcount"].sum() == o["path_sample"].sum()
    # the labelled counts cover whole training chunks: one initial state per chunk, every base
    assert o["labelled_counts"][:8].sum() == n // bench.TRAIN
    assert o["labelled_counts"][120:].sum() == n // bench.TRAIN * bench.TRAIN
    # every island record (1-based beg1..end1, the reference's filter passed) is a run of
    # island-state bases of the dumped path inside its chunk, ended by a non-island base
    isl, path = o["islands"], o["path_sample"]
    assert len(isl) > 0
    assert np.all(isl[:, 1] - isl[:, 0] + 1 == isl[:, 2])
    assert np.all((isl[:, 0] - 1) // bench.DECODE == isl[:, 3]) and np.all(isl[:, 3] < 5)
    assert np.all(isl[:, 4] > 0.5) and np.all(isl[:, 5] > 0.6)
    for b1, e1 in isl[:, :2].astype(np.int64):
        assert path[b1 - 1:e1].all() and path[e1] == 0
