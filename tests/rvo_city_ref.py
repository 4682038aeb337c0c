"""rvo3d_rvo_vel_city in plain Python, rule by rule (include/rvo3d.h): scalar float64 operations in the stated order, every
product, sum and quotient on its own.  Rules 1-3 take the drone side as given - the candidates' values, live, cone, tc_min
and des are inputs - and are what the host program and the HIP kernel are compared against, bit for bit.  drone_side() is
a restatement of rvo3d_rvo_vel's drone part with numpy's asin / acos, for the closed loop on the CPU.  TALLY counts the
branches seen."""
import collections
import math

import numpy as np

import building_rows_ref as ref6
import building_rows_moving_ref as ref8

INF = math.inf
_div = ref6._div

# the branches of rule 2 (per passing building and live candidate) and the tiers of rule 3
BRANCHES = ("inside_a0", "inside_leaving", "disc_le0", "moving_away", "beyond_horizon", "over_roof", "descending_onto_roof",
            "blocked")
TALLY = collections.Counter()


def gate(p, b, reach=10.0, below=1.0):
    """Rule 1's gate: (passes, ex, ey); building_rows_ref.gate with reciprocal_vel_obs.preprocess's constants."""
    ok, ex, ey, _ = ref6.gate(p, b, reach, below)
    return bool(ok), ex, ey


def roots(ex, ey, wx, wy, R):
    """The planar part of rule 2: (hit, t_in, t_out, branch)."""
    a = wx * wx + wy * wy
    bq = (2.0 * ex) * wx + (2.0 * ey) * wy
    cq = (ex * ex + ey * ey) - R * R
    if cq <= 0.0:
        if a == 0.0:
            return True, 0.0, INF, "inside_a0"
        return True, 0.0, _div(-bq + math.sqrt(bq * bq - (4.0 * a) * cq), 2.0 * a), "inside_leaving"
    disc = bq * bq - (4.0 * a) * cq
    if disc <= 0.0:
        return False, 0.0, 0.0, "disc_le0"
    s = math.sqrt(disc)
    t_in, t_out = _div(-bq - s, 2.0 * a), _div(-bq + s, 2.0 * a)
    if not t_in >= 0.0:
        return False, 0.0, 0.0, "moving_away"
    return True, t_in, t_out, None


def blocks(t_in, t_out, pz, cz, H, horizon):
    """The height part of rule 2: (blocks, branch)."""
    if not t_in <= horizon:
        return False, "beyond_horizon"
    te = t_out if t_out < horizon else horizon
    z_in, z_e = pz + cz * t_in, pz + cz * te
    zmin = z_e if z_e < z_in else z_in
    if not zmin <= H:
        return False, "over_roof"
    return True, ("descending_onto_roof" if z_in > H else "blocked")


def sweep(p, r, vals, cnt, live, buildings, vel_of, horizon=5.0, reach=10.0, below=1.0, clear_xy=0.0, clear_z=0.0,
          tally=TALLY):
    """Rules 1 and 2 for one drone.  vals: three lists of candidate values per axis, cnt their lengths, candidate
    c = (ix * cnt[1] + iy) * cnt[2] + iz; vel_of(i) -> (vb_x, vb_y, ...) of building i.  Returns (blocked mask, n_gated,
    tb: dict c -> minimum t_in over the buildings that block c)."""
    p, r = [float(x) for x in p], float(r)
    blocked, n_gated, tb = 0, 0, {}
    for i, b in enumerate(np.asarray(buildings, dtype=np.float64).reshape(-1, 4).tolist()):
        ok, ex, ey = gate(p, b, reach, below)
        if not ok:
            continue
        n_gated += 1
        vb = vel_of(i)
        R, H = (r + b[3]) + clear_xy, b[2] + clear_z
        for ix in range(cnt[0]):
            wx = vals[0][ix] - vb[0]
            for iy in range(cnt[1]):
                wy = vals[1][iy] - vb[1]
                hit, t_in, t_out, br = roots(ex, ey, wx, wy, R)
                for iz in range(cnt[2]):
                    c = (ix * cnt[1] + iy) * cnt[2] + iz
                    if not (live >> c) & 1:
                        continue
                    if not hit:
                        tally[br] += 1
                        continue
                    if br is not None:
                        tally[br] += 1
                    yes, br2 = blocks(t_in, t_out, p[2], vals[2][iz], H, horizon)
                    tally[br2] += 1
                    if yes:
                        blocked |= 1 << c
                        tb[c] = t_in if t_in < tb.get(c, INF) else tb[c]
    return blocked, n_gated, tb


def dist(des, v):
    ax, ay, az = des[0] - v[0], des[1] - v[1], des[2] - v[2]
    return math.sqrt(ax * ax + ay * ay + az * az)


def select(vals, cnt, live, cone, blocked, tb, tc_min, des, tally=TALLY):
    """Rule 3: (tier, velocity [3])."""
    des = [float(x) for x in des]
    cands = [(c, (vals[0][ix], vals[1][iy], vals[2][iz]))
             for ix in range(cnt[0]) for iy in range(cnt[1]) for iz in range(cnt[2])
             for c in [(ix * cnt[1] + iy) * cnt[2] + iz]]
    free = live & ~blocked
    t1 = [(c, v) for c, v in cands if (free & ~cone) >> c & 1]
    t2 = [(c, v) for c, v in cands if free >> c & 1]
    t3 = [(c, v) for c, v in cands if live >> c & 1]
    if t1:
        best = None
        for c, v in t1:
            dd = dist(des, v)
            if best is None or dd < best[0]:
                best = (dd, v)
        tally["tier1"] += 1
        return 1, list(best[1])
    if t2:
        tc_inv = INF if tc_min == 0 else _div(1.0, tc_min)
        best = None
        for c, v in t2:
            pen = 1 * tc_inv + dist(des, v)
            if best is None or pen < best[0]:
                best = (pen, v)
        tally["tier2"] += 1
        return 2, list(best[1])
    if t3:
        best = None
        for c, v in t3:
            dd = dist(des, v)
            if best is None or tb[c] > best[0] or (tb[c] == best[0] and dd < best[1]):
                best = (tb[c], dd, v)
        tally["tier3"] += 1
        return 3, list(best[2])
    tally["tier4"] += 1
    return 4, [0.0, 0.0, 0.0]


def candidates(v, vmax=(2.0, 2.0, 2.0), acceler=0.5):
    """Rule 0's candidate values: (vals, cnt, live) - np.arange(lo, hi, 0.5) per axis inside np.clip, at most four values
    (acceler <= 1), live bit c: |candidate| >= 0.3."""
    vals = []
    for k in range(3):
        lo, hi = np.clip(v[k] - acceler, -vmax[k], vmax[k]), np.clip(v[k] + acceler, -vmax[k], vmax[k])
        vals.append([float(x) for x in np.arange(lo, hi, 0.5)[:4]])
    cnt = [len(x) for x in vals]
    live = 0
    for ix in range(cnt[0]):
        for iy in range(cnt[1]):
            for iz in range(cnt[2]):
                x, y, z = vals[0][ix], vals[1][iy], vals[2][iz]
                if not math.sqrt(x * x + y * y + z * z) < 0.3:
                    live |= 1 << ((ix * cnt[1] + iy) * cnt[2] + iz)
    return vals, cnt, live


def drone_side(i, pos, vel, radius, prio, vals, cnt, live):
    """rvo3d_rvo_vel's cone set and tc_min for drone i of one env (pos, vel [N, 3]), with numpy's asin / acos: the
    reference's own sequence (get_alpha, get_PAA, get_beta, cal_exp_tim) for every candidate."""
    cone, tc_min = 0, INF
    p, v = pos[i], vel[i]
    for j in range(len(pos)):
        if j == i:
            continue
        f = p - pos[j]
        if not np.linalg.norm(f) <= 10.0:
            continue
        w, r = v - vel[j], radius[i] + radius[j]
        tc = ref6.INF
        qa, qb, qc = float(w @ w), float(2 * f @ w), float(f @ f) - r * r
        if qc <= 0:
            tc = 0.0
        else:
            temp = qb * qb - 4 * qa * qc
            if temp > 0:
                ts = [t for t in (_div(-qb + math.sqrt(temp), 2 * qa), _div(-qb - math.sqrt(temp), 2 * qa)) if t >= 0]
                tc = min(ts) if ts else INF
        tc_min = tc if tc < tc_min else tc_min
        a = pos[j] - p
        nab = float(np.linalg.norm(a))
        q = _div(r, nab)
        alpha = round(float(np.arcsin(q)), 2) if q <= 1.0 else 1.57
        pr = prio[i] / (prio[i] + prio[j])
        pa = pr * (2 * p + (v + vel[j]) * 1)
        for ix in range(cnt[0]):
            for iy in range(cnt[1]):
                for iz in range(cnt[2]):
                    c = (ix * cnt[1] + iy) * cnt[2] + iz
                    if not (live >> c) & 1:
                        continue
                    ww = (p + np.array([vals[0][ix], vals[1][iy], vals[2][iz]]) * 1) - pa
                    AB = nab * float(np.linalg.norm(ww))
                    cs = float(a @ ww) / AB if AB != 0 else 0.0
                    with np.errstate(invalid="ignore"):
                        beta = float(np.rint(np.arccos(cs) * 100.0) / 100.0)
                    if alpha > beta:
                        cone |= 1 << c
    return cone, tc_min


def rvo_city_ref(pos, vel, radius, buildings, live, cone, tc_min, des, motion=None, dt=1.0, vmax=(2.0, 2.0, 2.0),
                 acceler=0.5, horizon=5.0, reach=10.0, below=1.0, clear_xy=0.0, clear_z=0.0, counts=None,
                 building_counts=None, tally=TALLY):
    """The whole call from the device's own live / cone / tc_min / des.  pos, vel, des [E, N, 3], radius [E, N] or a scalar,
    live, cone [E, N] integers, tc_min [E, N], buildings [nb, 4] (shared; motion must be None) or [E, nb_max, 4] with
    building_counts [E] (None: all), motion: None or (ends, speed, leg), counts [E]: the live drones of a counted handle
    -> dict(out_vel [E, N, 3], blocked_mask [E, N] uint64, n_gated, tier [E, N] int32, live_mask: the restatement's own).
    Ghost rows are zeros."""
    pos, vel, des = (np.asarray(x, dtype=np.float64) for x in (pos, vel, des))
    E, N = pos.shape[:2]
    radius = np.broadcast_to(np.asarray(radius, dtype=np.float64), (E, N))
    bld = np.zeros((0, 4)) if buildings is None else np.asarray(buildings, dtype=np.float64)
    assert motion is None or bld.ndim == 3
    out = dict(out_vel=np.zeros((E, N, 3)), blocked_mask=np.zeros((E, N), np.uint64), n_gated=np.zeros((E, N), np.int32),
               tier=np.zeros((E, N), np.int32), live_mask=np.zeros((E, N), np.uint64))
    for e in range(E):
        be = bld if bld.ndim == 2 else bld[e, :(bld.shape[1] if building_counts is None else int(building_counts[e]))]
        if motion is None:
            vel_of = lambda i: (0.0, 0.0, 0)
        else:
            ends, speed, leg = (np.asarray(m)[e] for m in motion)
            vel_of = lambda i, be=be, ends=ends, speed=speed, leg=leg: ref8.velocity(be[i], ends[i], speed[i], leg[i], dt)
        for d in range(N if counts is None else int(counts[e])):
            vals, cnt, lv = candidates(vel[e, d], vmax, acceler)
            out["live_mask"][e, d] = lv
            lv_dev = int(live[e, d]) & (2 ** 64 - 1)
            blocked, n_gated, tb = sweep(pos[e, d], radius[e, d], vals, cnt, lv_dev, be, vel_of, horizon, reach, below,
                                         clear_xy, clear_z, tally)
            tier, v = select(vals, cnt, lv_dev, int(cone[e, d]) & (2 ** 64 - 1), blocked, tb, float(tc_min[e, d]),
                             des[e, d], tally)
            out["out_vel"][e, d], out["blocked_mask"][e, d] = v, blocked
            out["n_gated"][e, d], out["tier"][e, d] = n_gated, tier
    return out
