"""bench.py --dump-outputs and the plain (not --full) result line: the arrays of the last timed step are written as
float32 .npy files under the size cap, on a fixed seeded sample of envs when the batch is larger, and two runs with
the same arguments write the same arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _outs(E, N, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((E, N, W), generator=g), torch.randint(0, 11, (E, N), generator=g, dtype=torch.int32),
            torch.randn((E, N), generator=g), torch.randint(0, 2, (E, N), generator=g, dtype=torch.uint8),
            torch.randint(0, 2, (E, N), generator=g, dtype=torch.uint8), torch.randint(0, 2, (E, N), generator=g, dtype=torch.uint8))


def _load(d):
    return {n: np.load(os.path.join(d, n + ".npy")) for n in bench.DUMP_NAMES}


def test_dump_writes_every_output_as_float32(tmp_path):
    outs = _outs(8, 4, 102)
    rec = bench.dump_outputs(str(tmp_path), outs)
    got = _load(str(tmp_path))
    assert rec["envs"] == rec["of_envs"] == 8
    for n, t in zip(bench.DUMP_NAMES, outs):
        assert got[n].dtype == np.float32
        np.testing.assert_array_equal(got[n], t.numpy().astype(np.float32))


def test_dump_of_a_large_batch_is_a_fixed_sample_under_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 200_000)
    outs = _outs(64, 8, 102)
    a, b = tmp_path / "a", tmp_path / "b"
    rec = bench.dump_outputs(str(a), outs)
    bench.dump_outputs(str(b), outs)
    assert 0 < rec["envs"] < 64
    size = sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a))
    assert size <= 200_000 + 128 * len(bench.DUMP_NAMES)  # + the .npy headers
    ga, gb = _load(str(a)), _load(str(b))
    idx = np.sort(np.random.default_rng(1234).choice(64, rec["envs"], replace=False))
    for n, t in zip(bench.DUMP_NAMES, outs):
        np.testing.assert_array_equal(ga[n], gb[n])
        np.testing.assert_array_equal(ga[n], t.numpy()[idx].astype(np.float32))


def _bench(args):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_times_the_steps_asked_for_and_dumps_the_same_outputs_twice(tmp_path):
    args = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--prewarm", "2", "--envs", "32", "--drones", "16",
            "--map", "20", "20", "8"]
    recs = [_bench(args + ["--dump-outputs", str(tmp_path / d)]) for d in ("a", "b")]
    for rec in recs:
        assert rec["steps"] == 3 and rec["ms_per_step"] > 0 and rec["value"] > 0
        assert rec["dtype"] == "f64" and rec["higher_is_better"] is True
        assert not ({"roofline", "rollout", "cpu_baseline"} & set(rec))
        assert rec["outputs_dumped"]["envs"] == 32
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert a["obs"].shape == (32, 16, 102)
    for n in bench.DUMP_NAMES:
        np.testing.assert_array_equal(a[n], b[n])
