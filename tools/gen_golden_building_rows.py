#!/usr/bin/env python
"""tests/golden/calls_building_rows.npz: what the reference's own functions say about drones next to buildings.

    python tools/gen_golden_building_rows.py --reference /path/to/the/reference [--out tests/golden/calls_building_rows.npz]

Runs the reference alone (no GPU, nothing of this package): rvo_inter.preprocess (rvo_inter.py:85-107) gives, per drone,
the buildings it keeps for the observation; rvo_inter.cal_exp_tim_with_building (:248-275) the time to each building's
cylinder.  Seeded states with continuous-uniform coordinates (not rounded to two decimals), speeds up to 2, some zero
velocities, some drones inside a cylinder, plus a handful of exact cases: offset (3, 4) - d == 5.0 exactly, kept - and
h_b == p_z - 2 exactly - not kept.  The file name starts with calls_ like the other call-level vectors: the scenario replays (tests/golden_util.py:
scenario_files) leave those out.  Recorded: the inputs, the kept index lists (as a [drones, buildings] mask) and t.
tests/test_building_rows_host.py compares tests/building_rows_ref.py with it and prints how many pairs sit too close to a
threshold to be compared; this script prints the same count when generating (it must stay below 1 %)."""
import argparse
import os
import sys

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference project")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden",
                                                  "calls_building_rows.npz"))
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    from uaisa_env.vel_obs.rvo_inter import rvo_inter
    ri = rvo_inter()

    rng = np.random.default_rng(20240607)
    nd, nb = 200, 30
    bld = np.concatenate([rng.uniform(0.0, 40.0, (nb, 2)), rng.uniform(0.5, 12.0, (nb, 1)), rng.uniform(0.3, 2.5, (nb, 1))],
                         axis=1)
    # drones around the buildings, so that the 5 m gate is met often
    near = rng.integers(0, nb, nd)
    pos = np.concatenate([bld[near, :2] + rng.uniform(-7.0, 7.0, (nd, 2)), rng.uniform(0.0, 14.0, (nd, 1))], axis=1)
    ang, spd = rng.uniform(0.0, 2 * np.pi, nd), rng.uniform(0.0, 2.0, nd)
    vel = np.stack([spd * np.cos(ang), spd * np.sin(ang), rng.uniform(-1.0, 1.0, nd)], axis=1)
    vel[::9] = 0.0                                                  # some stand still
    aim = np.arange(3, nd, 7)                                       # some fly straight at their building
    to = bld[near[aim], :2] - pos[aim, :2]
    vel[aim, :2] = to / np.linalg.norm(to, axis=1, keepdims=True) * spd[aim, None]
    inside = np.arange(5, nd, 11)                                   # some are inside a cylinder
    pos[inside, :2] = bld[near[inside], :2] + bld[near[inside], 3:4] * rng.uniform(-0.6, 0.6, (len(inside), 2))
    rad = rng.uniform(0.1, 0.4, nd)
    # the exact cases: buildings at integer places, drones at exact offsets
    bld[0] = [10.0, 20.0, 6.0, 1.0]
    bld[1] = [30.0, 8.0, 4.0, 0.5]
    pos[0] = [13.0, 24.0, 3.0]; vel[0] = [-0.75, -1.0, 0.0]      # offset (3, 4): d == 5.0, kept; flying at it
    pos[1] = [7.0, 16.0, 7.5]; vel[1] = [0.0, 0.0, 0.0]          # offset (-3, -4), above the roof by 1.5: kept
    pos[2] = [30.0, 8.5, 6.0]; vel[2] = [1.0, 0.0, 0.0]          # h_b == p_z - 2 exactly: not kept
    pos[3] = [30.0, 8.5, 5.999999999999]; vel[3] = [1.0, 0.0, 0.0]  # just below that: kept
    rad[:4] = 0.25

    kept = np.zeros((nd, nb), dtype=bool)
    t = np.zeros((nd, nb))
    for i in range(nd):
        state = [pos[i, 0], pos[i, 1], pos[i, 2], vel[i, 0], vel[i, 1], vel[i, 2], rad[i]]
        _, obs_b = ri.preprocess(state, [], [list(b) for b in bld])
        for b in obs_b:
            j = int(np.flatnonzero((bld == np.asarray(b)).all(axis=1))[0])
            kept[i, j] = True
        for j in range(nb):
            t[i, j] = ri.cal_exp_tim_with_building(pos[i, 0] - bld[j, 0], pos[i, 1] - bld[j, 1], vel[i, 0], vel[i, 1],
                                                   rad[i] + bld[j, 3])
    assert kept[0, 0] and kept[1, 0] and not kept[2, 1] and kept[3, 1]

    # how many pairs sit within 1e-9 of a gate threshold (what the test leaves out)
    d = np.hypot(pos[:, None, 0] - bld[None, :, 0], pos[:, None, 1] - bld[None, :, 1])
    close = (np.abs(d - 5.0) <= 1e-9) | (np.abs(bld[None, :, 2] - (pos[:, None, 2] - 2.0)) <= 1e-9)
    print(f"{nd} drones x {nb} buildings: kept {int(kept.sum())}, t == 0: {int((t == 0).sum())}, "
          f"finite t > 0: {int((np.isfinite(t) & (t > 0)).sum())}, within 1e-9 of a gate: {int(close.sum())} "
          f"({100.0 * close.mean():.3f} %)")
    assert close.mean() <= 0.01
    np.savez_compressed(a.out, pos=pos, vel=vel, radius=rad, buildings=bld, kept=kept, t=t,
                        exact_pairs=np.array([[0, 0], [1, 0], [2, 1], [3, 1]], dtype=np.int32))
    print("wrote", os.path.normpath(a.out), os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
