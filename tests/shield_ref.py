"""rvo3d_shield_action in plain Python, rule by rule (include/rvo3d.h, S1-S6; csrc/rvo3d_shield_rules.hpp and
csrc/rvo3d_orca_rules.hpp are the statements the device compiles).  The plane of a pair, the programs, the gate and the
converter are tests/orca_ref.py's; the plane list is restated here with the per-neighbour share (S2).  One drone at a time,
scalar float64 operations in the stated order.  S1 goes through math.sin / math.cos and the converter through math.atan2 /
math.asin: against the device those two agree to orca_ref.CONVERTER_TOL, everything else is held to the bit once the
restatement is given the preferred velocity of the side it is compared with."""
import fractions
import math

import numpy as np

from orca_ref import CONVERTER_TOL, dot, gate, plane, solve, vel_command   # noqa: F401  (CONVERTER_TOL: for the tests)

DEG2RAD = 0.017453292519943295
INTERVENED = 8                       # flags: 8 | the command's clipped bits 1, 2, 4
TOTALS = ("judged", "intervened", "fallback", "clipped")


def fma(a, b, c):
    """a * b + c rounded once (exact rational arithmetic, then one rounding)."""
    return float(fractions.Fraction(a) * fractions.Fraction(b) + fractions.Fraction(c))


def clamp(x, lo, hi):
    return lo if x < lo else (hi if x > hi else x)


# ---- S1 ----
def pref_of(v, yaw, pitch, a):
    """The velocity behind the step of a drone that is not parked, for the action a."""
    vx, vy, vz = (float(x) for x in v)
    speed = math.sqrt(fma(vz, vz, fma(vy, vy, vx * vx)))
    acc = clamp(float(a[0]) * 1.0, -1.0, 1.0)
    dyaw = clamp(float(a[1]) * 90.0, -90.0, 90.0)
    dpit = clamp(float(a[2]) * 90.0, -90.0, 90.0)
    nv = speed + acc
    speed = 0.0 if 0.0 > nv else nv
    yaw = (float(yaw) + dyaw) % 360.0          # (a float's % is npy_divmod's remainder: the sign of the divisor)
    pitch = clamp(float(pitch) + dpit, -90.0, 90.0)
    sy, cy = math.sin(yaw * DEG2RAD), math.cos(yaw * DEG2RAD)
    sp, cp = math.sin(pitch * DEG2RAD), math.cos(pitch * DEG2RAD)
    return (speed * cp * cy, speed * cp * sy, speed * sp)


# ---- S2: orca_ref.planes_of with the share of every neighbour ----
def planes_of(i, pos, vel, rad, dest, n_live, buildings, vel_of, time_horizon=5.0, time_step=1.0, neighbor_dist=10.0,
              max_neighbors=10, max_buildings=4, reach=10.0, below=1.0, clear_xy=0.0, parked_share=1.0):
    """Drone i's planes, buildings first -> (planes, n_buildings kept).  dest [N]: the parked drones - drone i's share against
    such a neighbour is parked_share (the rule: 1; 0.5 is what the tests fly to show the difference)."""
    p = [float(x) for x in pos[i]]
    v = tuple(float(x) for x in vel[i])
    r = float(rad[i])
    nd2 = neighbor_dist * neighbor_dist
    near = []
    for j in range(n_live):
        if j == i:
            continue
        rel = (float(pos[j][0]) - p[0], float(pos[j][1]) - p[1], float(pos[j][2]) - p[2])
        d2 = dot(rel, rel)
        if d2 < nd2:
            near.append((d2, j))
    near.sort()
    near = near[:max_neighbors]
    blds = []
    for j, b in enumerate(buildings):
        ok, gap = gate(p, r, [float(x) for x in b], reach, below)
        if ok:
            blds.append((gap, j))
    blds.sort()
    blds = blds[:max_buildings]
    out = []
    for _, j in blds:
        b = [float(x) for x in buildings[j]]
        vb = vel_of(j)
        pp, pn, _ = plane((b[0] - p[0], b[1] - p[1], 0.0), (v[0] - float(vb[0]), v[1] - float(vb[1]), 0.0),
                          (r + b[3]) + clear_xy, time_horizon, time_step, 1.0, v)
        out.append((pp, pn))
    for _, j in near:
        rel = (float(pos[j][0]) - p[0], float(pos[j][1]) - p[1], float(pos[j][2]) - p[2])
        w_rel = (v[0] - float(vel[j][0]), v[1] - float(vel[j][1]), v[2] - float(vel[j][2]))
        share = parked_share if dest[j] else 0.5
        pp, pn, _ = plane(rel, w_rel, r + float(rad[j]), time_horizon, time_step, share, v)
        out.append((pp, pn))
    return out, len(blds)


def shield_env(pos, vel, yaw, pitch, rad, dest, n_live, action, buildings, vel_of=None, pref=None, max_speed=2.0, **kw):
    """One env, S1-S6 -> dict(out_action, pref_vel, out_vel [N][3]; status int32, flags uint8, slack [N]; totals int64 [4];
    planes: a list per row, None where the row is not judged).  pref [N][3]: the preferred velocities to take in place of
    S1's (the rows that are judged) - how the device's and the host program's S2-S6 are held to the bit."""
    N = len(pos)
    vel_of = vel_of or (lambda j: (0.0, 0.0))
    action = np.asarray(action, dtype=np.float64)
    out = dict(out_action=action.copy(), pref_vel=np.zeros((N, 3)), out_vel=np.zeros((N, 3)), status=np.zeros(N, np.int32),
               flags=np.zeros(N, np.uint8), slack=np.zeros(N), totals=np.zeros(4, np.int64), planes=[None] * N)
    out["out_action"][n_live:] = 0.0                                  # S5: a ghost's row
    for i in range(n_live):
        a = action[i]
        if dest[i] or not all(math.isfinite(float(x)) for x in a):    # S5
            continue
        planes, kb = planes_of(i, pos, vel, rad, dest, n_live, buildings, vel_of, **kw)
        pv = tuple(float(x) for x in pref[i]) if pref is not None else pref_of(vel[i], yaw[i], pitch[i], a)
        v, status, slack = solve(planes, kb, max_speed, pv)
        flags = 0
        if v[0] != pv[0] or v[1] != pv[1] or v[2] != pv[2]:           # S4
            cmd, bits = vel_command(vel[i], yaw[i], pitch[i], v)
            out["out_action"][i] = cmd
            flags = INTERVENED | bits
        out["pref_vel"][i], out["out_vel"][i], out["status"][i], out["flags"][i], out["slack"][i] = pv, v, status, flags, slack
        out["planes"][i] = planes
        out["totals"] += [1, flags != 0, status == 3, (flags & INTERVENED) != 0 and (flags & 7) != 0]   # S6
    return out
