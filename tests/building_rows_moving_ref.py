"""rvo3d_building_rows_moving in plain Python, rule by rule (include/rvo3d.h), on top of building_rows_ref.py: scalar
float64 operations in the stated order, every product, sum and quotient on its own.  What the host program and the HIP
kernel are compared against, bit for bit.  The buildings' positions come from building_motion_ref.move."""
import math

import numpy as np

import building_rows_ref as ref

r2 = ref.r2


def velocity(b, ends, speed, leg, dt):
    """Rule 2 for one record: (vb_x, vb_y, branch) - branch 0: static (ends is not read), 1: arrival (d <= step),
    2: cruise.  ends [2][2], or None when there is no motion."""
    if ends is None:
        return 0.0, 0.0, 0
    s, dt = float(speed), float(dt)
    step = s * dt
    if not step > 0.0:
        return 0.0, 0.0, 0
    T = ends[int(leg) & 1]
    dx, dy = float(T[0]) - float(b[0]), float(T[1]) - float(b[1])
    d = math.sqrt(dx * dx + dy * dy)
    if d <= step:
        return ref._div(dx, dt), ref._div(dy, dt), 1
    return ref._div(dx, d) * s, ref._div(dy, d) * s, 2


def pair(p, v, r, b, vb, reach=5.0, below=2.0):
    """building_rows_ref.pair with the building moving at vb: dict(..., t, urg: static; t_rel, urg_rel, c, disc, branch: at
    the relative velocity; row [8] float32)."""
    q = ref.pair(p, v, r, b, reach, below)
    p, v, b, r = [float(x) for x in p], [float(x) for x in v], [float(x) for x in b], float(r)
    t, c, disc, branch = ref.exp_time(p[0] - b[0], p[1] - b[1], v[0] - vb[0], v[1] - vb[1], r + b[3])
    urg = 1.0 / (t + 0.2)
    row = np.concatenate([q["row"][:5], np.array([r2(urg), r2(vb[0]), r2(vb[1])], dtype=np.float32)])
    q.update(t_rel=t, urg_rel=urg, c=c, disc=disc, branch=branch, row=row, row6=q["row"])
    return q


def drone_rows(p, v, r, buildings, k, vel_of, reach=5.0, below=2.0):
    """Rules 1-5 for one drone.  vel_of(i) -> (vb_x, vb_y, branch) of building i.  Returns (rows [k, 8] float32, count,
    kept indices, per kept row dict(branch, urg6: r2 of the static urg as float32))."""
    _, cnt, kept = ref.drone_rows(p, v, r, buildings, k, reach, below)
    bl = np.asarray(buildings, dtype=np.float64).reshape(-1, 4)
    rows = np.zeros((k, 8), dtype=np.float32)
    info = []
    for s, i in enumerate(kept):
        vbx, vby, br = vel_of(i)
        q = pair(p, v, r, bl[i], (vbx, vby), reach, below)
        rows[s] = q["row"]
        info.append(dict(index=i, branch=br, urg6=q["row6"][5], urg8=q["row"][5]))
    return rows, cnt, kept, info


def building_rows_moving_ref(pos, vel, radius, buildings, k, motion=None, dt=1.0, reach=5.0, below=2.0, counts=None,
                             building_counts=None):
    """pos, vel [E, N, 3], radius [E, N] or a scalar, buildings [nb, 4] (shared; motion must be None) or [E, nb_max, 4] with
    building_counts [E] (None: all), motion: None or (ends [E, nb_max, 2, 2], speed [E, nb_max], leg [E, nb_max]), counts
    [E]: the live drones of a counted handle -> (rows [E, N, k, 8] float32, b_count [E, N] int32, tally, branch), tally:
    dict of counts over the kept rows - kept, moving, arrival, urg_differs (r2(urg_rel) != r2(urg)), zero_to_positive;
    branch [E, N, k] int8: the velocity rule's branch of every kept row (0 static, 1 arrival, 2 cruise), -1 for an empty one."""
    pos, vel = np.asarray(pos, dtype=np.float64), np.asarray(vel, dtype=np.float64)
    E, N = pos.shape[:2]
    radius = np.broadcast_to(np.asarray(radius, dtype=np.float64), (E, N))
    bld = np.zeros((0, 4)) if buildings is None else np.asarray(buildings, dtype=np.float64)
    assert motion is None or bld.ndim == 3
    rows = np.zeros((E, N, k, 8), dtype=np.float32)
    cnt = np.zeros((E, N), dtype=np.int32)
    tally = dict(kept=0, moving=0, arrival=0, urg_differs=0, zero_to_positive=0)
    branch = np.full((E, N, k), -1, dtype=np.int8)
    for e in range(E):
        be = bld if bld.ndim == 2 else bld[e, :(bld.shape[1] if building_counts is None else int(building_counts[e]))]
        if motion is None:
            vel_of = lambda i: (0.0, 0.0, 0)
        else:
            ends, speed, leg = (np.asarray(m)[e] for m in motion)
            cache = {}

            def vel_of(i, be=be, ends=ends, speed=speed, leg=leg, cache=cache):
                if i not in cache:
                    cache[i] = velocity(be[i], ends[i], speed[i], leg[i], dt)
                return cache[i]
        for d in range(N if counts is None else int(counts[e])):
            rows[e, d], cnt[e, d], _, info = drone_rows(pos[e, d], vel[e, d], radius[e, d], be, k, vel_of, reach, below)
            for s, q in enumerate(info):
                branch[e, d, s] = q["branch"]
                tally["kept"] += 1
                tally["moving"] += q["branch"] != 0
                tally["arrival"] += q["branch"] == 1
                tally["urg_differs"] += bool(q["urg6"] != q["urg8"])
                tally["zero_to_positive"] += bool(q["urg6"] == 0 and q["urg8"] > 0)
    return rows, cnt, tally, branch
