"""bench.py's command line: a plain run times the training jobs only (the
legs with runs of their own are behind --full), --steps sets the number of
timed jobs, and --dump-outputs writes the last timed job's merges and ids."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_lib as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

FILES = {"merges.npy": np.float64, "ids_head.npy": np.float32, "ids_sample_index.npy": np.float64,
         "ids_sample.npy": np.float32, "ids_digest.npy": np.float64}
FULL_ONLY = ("train_1024", "ingest", "config1", "cpu_baseline", "cpu_baseline_1g", "encode")


def _load(d):
    assert sorted(os.listdir(d)) == sorted(FILES)
    out = {f: np.load(os.path.join(d, f)) for f in FILES}
    for f, dt in FILES.items():
        assert out[f].dtype == dt, f
    return out


def _check(got, merges, ids, n_ids, csum):
    assert (got["merges.npy"] == merges).all() and got["merges.npy"].shape == merges.shape
    assert (got["ids_head.npy"] == ids[:bench.DUMP_HEAD]).all()
    idx = got["ids_sample_index.npy"].astype(np.int64)
    assert idx.size == min(ids.size, idx.size) and (np.diff(idx) > 0).all() and 0 <= idx[0] and idx[-1] < ids.size
    assert (got["ids_sample.npy"] == ids[idx]).all()
    assert got["ids_digest.npy"].tolist() == [n_ids, csum >> 32, csum & 0xFFFFFFFF]


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path):
    """more ids than the sample holds: the same seeded positions every time,
    every value exact in its float type, and the files' worst case (a full
    head and sample, 65536 merges) under 64 MB"""
    rng = np.random.default_rng(1)
    ids = rng.integers(0, 256 + 65536, bench.DUMP_SAMPLE + 12345, dtype=np.uint32)
    merges = rng.integers(0, 256 + 65536, (300, 2), dtype=np.uint32)
    csum = 0xFEDCBA9876543210
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), merges, ids, ids.size, csum)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    _check(a, merges, ids, ids.size, csum)
    assert all((a[f] == b[f]).all() for f in FILES)
    # S draws from n >= S positions leave at least (1 - 1/e) S distinct ones
    assert bench.DUMP_SAMPLE * 0.62 < a["ids_sample.npy"].size <= bench.DUMP_SAMPLE
    worst = bench.DUMP_HEAD * 4 + bench.DUMP_SAMPLE * (4 + 8) + 65536 * 2 * 8 + 3 * 8 + 5 * 128
    assert worst < 64e6
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in FILES) <= worst


def test_dump_outputs_small_job_is_whole(tmp_path):
    ids = np.arange(1000, dtype=np.uint32)[::-1].copy()
    merges = np.array([[97, 98], [256, 99]], dtype=np.uint32)
    bench.dump_outputs(str(tmp_path / "d"), merges, ids, ids.size, 7)
    got = _load(tmp_path / "d")
    _check(got, merges, ids, 1000, 7)
    assert (got["ids_sample_index.npy"] == np.arange(1000)).all()


def _run_bench(*argv):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_steps_and_dumps_the_last_job(tmp_path):
    """a small plain run (1 MiB, 64 merges): 3 timed jobs, none of the --full
    legs, and the dump equal to the same job run through the Python API"""
    from llmtokenizer_amd import api
    size, merges_n = 1 << 20, 64
    d = tmp_path / "out"
    line = _run_bench("--gpus", "1", "--steps", "3", "--warmup", "1", "--size", str(size), "--merges", str(merges_n),
                      "--dump-outputs", str(d))
    assert "error" not in line
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "corpus MB/s per merge iter" and line["higher_is_better"] is True and line["dtype"] == "u32"
    assert line["value"] == pytest.approx(size / 1e6 * merges_n / (line["ms_per_step"] * 1e-3), rel=1e-3)
    assert not [k for k in FULL_ONLY if k in line]
    e = api.Engine(0)
    e.synth(2, size)
    assert e.train(merges_n) == merges_n
    merges, ids = e.merges(), e.ids()
    e.close()
    csum = G.ids_checksum(ids)
    assert line["correctness"]["ids_checksum"] == "%016x" % csum
    _check(_load(d), merges, ids, ids.size, csum)
