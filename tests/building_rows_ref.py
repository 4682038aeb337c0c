"""rvo3d_building_rows in plain Python, rule by rule (include/rvo3d.h): scalar float64 operations in the stated order,
every product and sum on its own.  What the host program and the HIP kernel are compared against, bit for bit; it also
returns the unrounded d, gap and t of every pair, which the fixture of the reference's own functions is compared with."""
import math

import numpy as np

INF = math.inf


def r2(v):
    """np.round(v, 2) as numpy computes it, + 0.0 (no -0.0)."""
    return float(np.rint(np.float64(v) * 100.0)) / 100.0 + 0.0


def _div(x, y):
    with np.errstate(all="ignore"):
        return float(np.float64(x) / np.float64(y))


def gate(p, b, reach=5.0, below=2.0):
    """(passes, ex, ey, d) of rule 1."""
    ex, ey = p[0] - b[0], p[1] - b[1]
    d = math.sqrt(ex * ex + ey * ey)
    return (b[2] > p[2] - below) and (d <= reach), ex, ey, d


def exp_time(ex, ey, vx, vy, R):
    """Rule 3: (t, c, disc, branch) - branch 0: inside (t = 0), 1: never (t = inf, disc <= 0), 2: the roots decide."""
    a = vx * vx + vy * vy
    bq = (2.0 * ex) * vx + (2.0 * ey) * vy
    c = (ex * ex + ey * ey) - R * R
    if c <= 0.0:
        return 0.0, c, None, 0
    disc = bq * bq - (4.0 * a) * c
    if disc <= 0.0:
        return INF, c, disc, 1
    s = math.sqrt(disc)
    t1, t2 = _div(-bq + s, 2.0 * a), _div(-bq - s, 2.0 * a)
    t3 = t1 if t1 >= 0.0 else INF
    t4 = t2 if t2 >= 0.0 else INF
    return (t4 if t4 < t3 else t3), c, disc, 2


def pair(p, v, r, b, reach=5.0, below=2.0):
    """Everything about one (drone, building) pair: dict(passes, d, gap, t, urg, c, disc, branch, row [6] float32)."""
    p, v, b, r = [float(x) for x in p], [float(x) for x in v], [float(x) for x in b], float(r)
    ok, ex, ey, d = gate(p, b, reach, below)
    gap = d - (r + b[3])
    t, c, disc, branch = exp_time(ex, ey, v[0], v[1], r + b[3])
    urg = 1.0 / (t + 0.2)
    row = np.array([r2(b[0] - p[0]), r2(b[1] - p[1]), r2(b[2] - p[2]), r2(b[3]), r2(gap), r2(urg)], dtype=np.float32)
    return dict(passes=ok, d=d, gap=gap, t=t, urg=urg, c=c, disc=disc, branch=branch, row=row)


def drone_rows(p, v, r, buildings, k, reach=5.0, below=2.0, want_passing=False):
    """Rules 1-5 for one drone: (rows [k, 6] float32, count, kept building indices[, passing])."""
    p, r = [float(x) for x in p], float(r)
    bl = np.asarray(buildings, dtype=np.float64).reshape(-1, 4).tolist()
    cand = []
    for i, b in enumerate(bl):
        ok, _, _, d = gate(p, b, reach, below)
        if ok:
            cand.append((d - (r + b[3]), i))
    cand.sort()
    rows = np.zeros((k, 6), dtype=np.float32)
    for s, (_, i) in enumerate(cand[:k]):
        rows[s] = pair(p, v, r, bl[i], reach, below)["row"]
    out = (rows, min(k, len(cand)), [i for _, i in cand[:k]])
    return out + (len(cand),) if want_passing else out


def building_rows_ref(pos, vel, radius, buildings, k, reach=5.0, below=2.0, counts=None, building_counts=None):
    """pos, vel [E, N, 3], radius [E, N] or a scalar, buildings [nb, 4] (shared) or [E, nb_max, 4] with building_counts [E]
    (None: all), counts [E]: the live drones of a counted handle -> (rows [E, N, k, 6] float32, b_count [E, N] int32,
    passing [E, N] int32: how many buildings passed the gate)."""
    pos, vel = np.asarray(pos, dtype=np.float64), np.asarray(vel, dtype=np.float64)
    E, N = pos.shape[:2]
    radius = np.broadcast_to(np.asarray(radius, dtype=np.float64), (E, N))
    bld = np.zeros((0, 4)) if buildings is None else np.asarray(buildings, dtype=np.float64)
    rows = np.zeros((E, N, k, 6), dtype=np.float32)
    cnt = np.zeros((E, N), dtype=np.int32)
    passing = np.zeros((E, N), dtype=np.int32)
    for e in range(E):
        be = bld if bld.ndim == 2 else bld[e, :(bld.shape[1] if building_counts is None else int(building_counts[e]))]
        for d in range(N if counts is None else int(counts[e])):
            rows[e, d], cnt[e, d], _, passing[e, d] = drone_rows(pos[e, d], vel[e, d], radius[e, d], be, k, reach, below,
                                                                 want_passing=True)
    return rows, cnt, passing
