#!/usr/bin/env python
"""tests/golden/calls_building_time_rel.npz: what the reference's own cal_exp_tim_with_building says about drones next to
buildings that move, given the relative velocity it was written for.

    python tools/gen_golden_building_time_rel.py --reference /path/to/the/reference [--out tests/golden/calls_building_time_rel.npz]

Runs the reference alone (no GPU, nothing of this package): rvo_inter.cal_exp_tim_with_building(ex, ey, v_x - vb_x,
v_y - vb_y, r + r_b) (rvo_inter.py:248-275) for every (drone, building) pair.  Drones and buildings are drawn as
tools/gen_golden_building_rows.py draws them (continuous-uniform coordinates, speeds up to 2, some zero velocities, some
drones inside a cylinder); every building gets a velocity with a speed ~U(0, 1.5) in a uniform direction, every fifth
stands still; then some buildings are planted: aimed straight at a drone that stands still (the static time is +inf, the
relative one finite), and moving exactly with their drone (zero relative velocity: +inf, where the static time is finite
for a drone flying at the building).  Recorded: the inputs, the velocities, t per pair and the planted pairs.
tests/test_building_rows_moving_host.py compares tests/building_rows_moving_ref.py with it; pairs whose c or disc lies
within 1e-9 of its scale are exempt there, as in tests/test_building_rows_host.py - this script counts them with the same
rule, prints the count and asserts that it stays at or below 1 % (a pair with zero relative velocity has scale 0 and is
decided, not exempt)."""
import argparse
import os
import sys

import numpy as np


def exempt(ex, ey, vx, vy, R):
    """The rule of the tests: True when c or disc sits within 1e-9 of its scale (float64, the reference's formulas)."""
    a, bq = vx ** 2 + vy ** 2, 2 * ex * vx + 2 * ey * vy
    c = ex * ex + ey * ey - R * R
    if not abs(c) > 1e-9 * (ex * ex + ey * ey + R * R):
        return True
    if c <= 0:
        return False
    disc = bq * bq - 4.0 * a * c
    scale = bq * bq + 4.0 * a * abs(c)
    return not (abs(disc) > 1e-9 * scale or scale == 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference project")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden",
                                                  "calls_building_time_rel.npz"))
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    from uaisa_env.vel_obs.rvo_inter import rvo_inter
    ri = rvo_inter()

    rng = np.random.default_rng(20240921)
    nd, nb = 200, 30
    bld = np.concatenate([rng.uniform(0.0, 40.0, (nb, 2)), rng.uniform(0.5, 12.0, (nb, 1)), rng.uniform(0.3, 2.5, (nb, 1))],
                         axis=1)
    near = rng.integers(0, nb, nd)
    pos = np.concatenate([bld[near, :2] + rng.uniform(-7.0, 7.0, (nd, 2)), rng.uniform(0.0, 14.0, (nd, 1))], axis=1)
    ang, spd = rng.uniform(0.0, 2 * np.pi, nd), rng.uniform(0.0, 2.0, nd)
    vel = np.stack([spd * np.cos(ang), spd * np.sin(ang), rng.uniform(-1.0, 1.0, nd)], axis=1)
    vel[::9] = 0.0                                                  # some stand still
    aim = np.arange(3, nd, 7)                                       # some fly straight at their building
    to = bld[near[aim], :2] - pos[aim, :2]
    vel[aim, :2] = to / np.linalg.norm(to, axis=1, keepdims=True) * np.maximum(spd[aim, None], 0.25)
    inside = np.arange(5, nd, 11)                                   # some are inside a cylinder
    pos[inside, :2] = bld[near[inside], :2] + bld[near[inside], 3:4] * rng.uniform(-0.6, 0.6, (len(inside), 2))
    rad = rng.uniform(0.1, 0.4, nd)

    # a velocity per building: speeds 0 .. 1.5, every fifth stands still
    bang, bspd = rng.uniform(0.0, 2 * np.pi, nb), rng.uniform(0.0, 1.5, nb)
    vb = np.stack([bspd * np.cos(bang), bspd * np.sin(bang)], axis=1)
    vb[::5] = 0.0
    # planted, each on a building of its own (not a standing one): aimed straight at a standing drone / moving with a drone
    # that flies at it.  The drone is outside the cylinder by 0.1 m at least.
    taken = set(range(0, nb, 5))
    aimed_pairs, with_pairs = [], []

    def outside(i, j):
        return np.hypot(*(pos[i, :2] - bld[j, :2])) > rad[i] + bld[j, 3] + 0.1

    for i in range(0, nd, 9):                                       # the standing drones
        j = int(near[i])
        if j not in taken and outside(i, j) and not vel[i, :2].any() and len(aimed_pairs) < 6:
            to = pos[i, :2] - bld[j, :2]
            vb[j] = to / np.linalg.norm(to) * (0.4 + 0.2 * len(aimed_pairs))
            taken.add(j)
            aimed_pairs.append((i, j))
    for i in aim:                                                   # the drones flying at their building
        j = int(near[i])
        if j not in taken and outside(i, j) and vel[i, :2].any() and len(with_pairs) < 6:
            vb[j] = vel[i, :2]
            taken.add(j)
            with_pairs.append((int(i), j))
    assert len(aimed_pairs) >= 4 and len(with_pairs) >= 4, (aimed_pairs, with_pairs)

    t = np.zeros((nd, nb))
    n_exempt = 0
    for i in range(nd):
        for j in range(nb):
            ex, ey, R = pos[i, 0] - bld[j, 0], pos[i, 1] - bld[j, 1], rad[i] + bld[j, 3]
            t[i, j] = ri.cal_exp_tim_with_building(ex, ey, vel[i, 0] - vb[j, 0], vel[i, 1] - vb[j, 1], R)
            n_exempt += exempt(ex, ey, vel[i, 0] - vb[j, 0], vel[i, 1] - vb[j, 1], R)
    for i, j in aimed_pairs:
        ex, ey, R = pos[i, 0] - bld[j, 0], pos[i, 1] - bld[j, 1], rad[i] + bld[j, 3]
        assert np.isinf(ri.cal_exp_tim_with_building(ex, ey, vel[i, 0], vel[i, 1], R)) and 0 < t[i, j] < np.inf, (i, j)
    for i, j in with_pairs:
        ex, ey, R = pos[i, 0] - bld[j, 0], pos[i, 1] - bld[j, 1], rad[i] + bld[j, 3]
        assert 0 < ri.cal_exp_tim_with_building(ex, ey, vel[i, 0], vel[i, 1], R) < np.inf and np.isinf(t[i, j]), (i, j)

    print(f"{nd} drones x {nb} buildings: t == 0: {int((t == 0).sum())}, finite t > 0: "
          f"{int((np.isfinite(t) & (t > 0)).sum())}, +inf: {int(np.isinf(t).sum())}, moving buildings "
          f"{int(vb.any(axis=1).sum())}, aimed pairs {len(aimed_pairs)}, with pairs {len(with_pairs)}, exempt (c or disc "
          f"within 1e-9 of its scale): {n_exempt} ({100.0 * n_exempt / (nd * nb):.3f} %)")
    assert n_exempt * 100 <= nd * nb
    np.savez_compressed(a.out, pos=pos, vel=vel, radius=rad, buildings=bld, building_vel=vb, t=t,
                        aimed_pairs=np.array(aimed_pairs, dtype=np.int32), with_pairs=np.array(with_pairs, dtype=np.int32))
    print("wrote", os.path.normpath(a.out), os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
