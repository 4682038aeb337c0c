"""The host-testable halves of the fused evaluation loop (rvo3d_amd.policy.post_train, fused=True), no GPU needed:

  * the per-env episode decision the accounting kernel calls (csrc/rvo3d_eval_kernels.hpp: eval_account_env) -
    tests/host/eval_account_check.hip is a stand-alone program that calls it and no HIP function, built here with
    AddressSanitizer and UndefinedBehaviorSanitizer on the host side and run as a child process;
  * the pure function that turns episode records into the evaluator's result (summarize_records), on the episodes the
    REFERENCE's policy_test produced (tests/golden/post_train_*.npz)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from golden_util import load

CSRC = os.path.join(ROOT, "3drvo-marl-collisionavoidance_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "eval_account_check.hip")
FLAGS = ["--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-O1",
         "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
POST_TRAIN = sorted(f for f in os.listdir(os.path.join(ROOT, "tests", "golden")) if f.startswith("post_train_"))


def test_eval_account_decision_under_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "eval_account_check")
    subprocess.check_call([hipcc] + FLAGS + ["-I", CSRC, "-o", exe, SRC])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(res.stdout)
    print(res.stderr)
    assert res.returncode == 0, res.stderr[-4000:]
    assert "eval account ok" in res.stdout


@pytest.mark.parametrize("name", POST_TRAIN)
def test_summary_of_the_references_episodes(name):
    """The reference's own episodes as records - the step each ended behind is the running sum of the lengths (E = 1:
    one episode after the other), handed over in shuffled order: the statistics are the fixture's, the lists come back in
    the order the episodes ended."""
    from rvo3d_amd.policy.post_train import REC_ARRIVED, REC_FINISHED, summarize_records
    fx = load(os.path.join(ROOT, "tests", "golden", name))
    n = len(fx["ep_len"])
    step = np.cumsum(fx["ep_len"].astype(np.int64)) - 1
    flags = (fx["ep_arrived"] * REC_ARRIVED + fx["ep_finished"] * REC_FINISHED).astype(np.uint8)
    ret = np.arange(n, dtype=np.float64) * 0.5 - 1.0     # (the fixture keeps no returns: any distinct values)
    perm = np.random.default_rng(5).permutation(n)
    assert not np.array_equal(perm, np.arange(n))
    got, line, lines = summarize_records(step[perm], np.zeros(n, np.int64), fx["ep_len"][perm], ret[perm],
                                         fx["ep_speed"][perm], flags[perm], policy_name="scripted")
    arrived = fx["ep_arrived"].astype(bool)
    assert got["episodes"] == n == int(fx["num_episodes"])
    assert got["ep_len"] == fx["ep_len"][arrived].tolist()
    assert got["speed"] == fx["ep_speed"].tolist()
    assert got["ep_ret"] == ret.tolist()
    assert got["success_rate"] == fx["ep_finished"].mean()
    for k in ("mean_len", "std_len", "average_speed", "std_speed"):
        assert got[k] == float(fx[k]), k
    assert len(lines) == n and all(ln.startswith("Successful" if a else "Fail") for ln, a in zip(lines, arrived))
    assert "Episode %d " % (n - 1) in lines[-1] and "EpLen %d " % fx["ep_len"][-1] in lines[-1]
    assert line.startswith("policy_name: scripted  successful rate: {:.2%}".format(fx["ep_finished"].mean()))


def test_summary_orders_by_step_then_env():
    """Episodes of several envs that ended behind the same step come in env order, as the sequential loop walks them."""
    from rvo3d_amd.policy.post_train import summarize_records
    step = np.array([7, 2, 7, 2, 5])
    env = np.array([2, 1, 0, 0, 1])
    length = np.array([3, 2, 8, 1, 4])
    got, _, lines = summarize_records(step, env, length, length * 1.0, length * 0.1, np.full(5, 3, np.uint8))
    assert got["ep_len"] == [1, 2, 4, 8, 3]
    assert got["ep_ret"] == [1.0, 2.0, 4.0, 8.0, 3.0]
    assert got["success_rate"] == 1.0 and got["episodes"] == 5
    assert [ln.split()[2] for ln in lines] == ["0", "1", "2", "3", "4"]
