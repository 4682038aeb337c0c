"""Moving buildings on the host (csrc/rvo3d_motion_kernels.hpp: motion_move, motion_cell; csrc/rvo3d_host_setup.hpp:
check_move_env_buildings): the rules move_buildings_kernel runs are __host__ __device__ functions, so the same text runs
here on the CPU.  After random moves the per-cell lists equal build_building_grid's u16 for u16 (3 x 3 and 1 x 1 cells,
fillers behind and between the live records, a cell that overflows and one that stops), a building reaches its endpoint
exactly and flips leg, speed 0 / NaN leave the record's bits alone, the argument checks refuse what they must.

The checks are C++: tests/host/building_motion_check.hip is a stand-alone program that calls the headers' functions and
no HIP function.  It is built here with AddressSanitizer and UndefinedBehaviorSanitizer on the host side and run as a
child process; no GPU is needed.  The trajectory it prints is compared, bit for bit, with tests/building_motion_ref.py:
the numpy reference the GPU tests use."""
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

from conftest import ROOT
import building_motion_ref as ref

CSRC = os.path.join(ROOT, "3drvo-marl-collisionavoidance_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "building_motion_check.hip")
FLAGS = ["--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-O1",
         "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]


@functools.lru_cache(maxsize=None)
def program_output():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "building_motion_check")
        subprocess.check_call([hipcc] + FLAGS + ["-I", CSRC, "-o", exe, SRC])
        res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print("\n".join(l for l in res.stdout.splitlines() if not l.startswith("traj")))
    print(res.stderr)
    assert res.returncode == 0, res.stderr[-4000:]
    return res.stdout


def test_building_motion_rules_under_sanitizers():
    assert "building motion ok" in program_output()


def f64(words):
    return np.array([int(w, 16) for w in words], dtype=np.uint64).view(np.float64)


def test_trajectory_equals_the_numpy_reference():
    lines = [l.split() for l in program_output().splitlines()]
    dt = f64([l[1] for l in lines if l[0] == "traj_dt"])[0]
    rows = [l for l in lines if l[0] == "traj_in"]
    nb = len(rows)
    assert nb == 12 and [int(l[1]) for l in rows] == list(range(nb))
    leg = np.array([int(l[2]) for l in rows], dtype=np.uint8)[None]
    bld = np.stack([f64(l[3:7]) for l in rows])[None]
    ends = np.stack([f64(l[7:11]) for l in rows]).reshape(1, nb, 2, 2)
    speed = np.stack([f64(l[11:12]) for l in rows]).reshape(1, nb)
    steps = [l for l in lines if l[0] == "traj"]
    T = len(steps) // nb
    assert T == 30 and len(steps) == T * nb
    flips, moved = 0, np.zeros(nb, bool)
    for t in range(T):
        new, new_leg = ref.move(bld, ends, speed, leg, dt)
        flips += int((new_leg != leg).sum())
        moved |= (new[0, :, :2] != bld[0, :, :2]).any(1)
        bld, leg = new, new_leg
        for b in range(nb):
            l = steps[t * nb + b]
            assert (int(l[1]), int(l[2])) == (t, b)
            got = f64(l[4:6])
            assert int(l[3]) == leg[0, b], (t, b)
            assert np.array_equal(got.view(np.uint64), bld[0, b, :2].view(np.uint64)), (t, b, got, bld[0, b, :2])
    assert flips >= 4 and moved.sum() == nb - 3, (flips, moved)   # the filler, speed 0 and the NaN speed stay
    assert not moved[[2, 5, 7]].any()
