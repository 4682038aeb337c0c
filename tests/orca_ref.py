"""rvo3d_orca_vel and rvo3d_vel_command in plain Python, rule by rule (include/rvo3d.h; csrc/rvo3d_orca_rules.hpp is the
statement the device compiles): scalar float64 operations in the stated order, every one rounded on its own, math.sqrt,
and for the converter math.atan2 / math.asin.  One drone at a time.  The GPU tests and tests/host/orca_check.hip are held
to these bits."""
import math

import numpy as np

EPS = 1e-5
INF = float("inf")
RAD2DEG = 57.29577951308232
# the largest |step(vel_command(w)) - w| that tests/test_orca_host.py::test_converter_against_the_step measures on its seeded
# inputs, through the oracle's kinematic step on the CPU, and the tolerance made of it: ten times that
CONVERTER_ERR = 7.58e-15
CONVERTER_TOL = 10 * CONVERTER_ERR


# ---- vectors: tuples of three floats ----
def add(a, b): return (a[0] + b[0], a[1] + b[1], a[2] + b[2])
def sub(a, b): return (a[0] - b[0], a[1] - b[1], a[2] - b[2])
def mul(s, a): return (s * a[0], s * a[1], s * a[2])
def div(a, s): return (a[0] / s, a[1] / s, a[2] / s)
def dot(a, b): return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
def cross(a, b): return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def unit(a, length):
    if not length > 0.0:
        return (1.0, 0.0, 0.0)
    return div(a, length)


# ---- rule 4 ----
def plane(rel, w_rel, R, tau, time_step, share, v_i):
    """-> (point, normal, branch); branch 0 cut-off circle, 1 leg, 2 overlapping."""
    d2, R2 = dot(rel, rel), R * R
    if d2 > R2:
        w = sub(w_rel, div(rel, tau))
        wl2, dp = dot(w, w), dot(w, rel)
        if dp < 0.0 and dp * dp > R2 * wl2:
            wl = math.sqrt(wl2)
            n = unit(w, wl)
            u = mul(R / tau - wl, n)
            br = 0
        else:
            a, b = d2, dot(rel, w_rel)
            cr = cross(rel, w_rel)
            c = dot(w_rel, w_rel) - dot(cr, cr) / (d2 - R2)
            disc = b * b - a * c
            if not disc > 0.0:
                disc = 0.0
            t = (b + math.sqrt(disc)) / a
            ww = sub(w_rel, mul(t, rel))
            wwl = math.sqrt(dot(ww, ww))
            if wwl > 0.0:
                n = div(ww, wwl)
            else:   # on the cone's axis: the normal towards e x rel
                e = (1.0, 0.0, 0.0) if rel[0] == 0.0 and rel[1] == 0.0 else (0.0, 0.0, 1.0)
                perp = cross(e, rel)
                pl, d = math.sqrt(dot(perp, perp)), math.sqrt(d2)
                n = sub(mul(math.sqrt(d2 - R2) / d, div(perp, pl)), mul(R / d, div(rel, d)))
            u = mul(R * t - wwl, n)
            br = 1
    else:
        w = sub(w_rel, div(rel, time_step))
        wl = math.sqrt(dot(w, w))
        n = unit(w, wl)
        u = mul(R / time_step - wl, n)
        br = 2
    return add(v_i, mul(share, u)), n, br


# ---- rule 6: planes are (point, normal) pairs ----
def lp1(planes, count, dirn, point, radius, opt, direction_opt):
    dp = dot(point, dirn)
    disc = (dp * dp + radius * radius) - dot(point, point)
    if not disc >= 0.0:
        return None
    sd = math.sqrt(disc)
    t_left, t_right = -dp - sd, -dp + sd
    for i in range(count):
        pp, pn = planes[i]
        num = dot(sub(pp, point), pn)
        den = dot(dirn, pn)
        if den * den <= EPS:
            if num > 0.0:
                return None
            continue
        t = num / den
        if den >= 0.0:
            t_left = t if t > t_left else t_left
        else:
            t_right = t if t < t_right else t_right
        if t_left > t_right:
            return None
    if direction_opt:
        t = t_right if dot(opt, dirn) > 0.0 else t_left
    else:
        t = dot(dirn, sub(opt, point))
        t = t_left if t < t_left else (t_right if t > t_right else t)
    return add(point, mul(t, dirn))


def lp2(planes, no, radius, opt, direction_opt):
    qp, qn = planes[no]
    dist = dot(qp, qn)
    dist2, r2 = dist * dist, radius * radius
    if dist2 > r2:
        return None
    pr2 = r2 - dist2
    centre = mul(dist, qn)
    if direction_opt:
        po = sub(opt, mul(dot(opt, qn), qn))
        l2 = dot(po, po)
        result = centre if l2 <= EPS else add(centre, mul(math.sqrt(pr2 / l2), po))
    else:
        result = add(opt, mul(dot(sub(qp, opt), qn), qn))
        if dot(result, result) > r2:
            pres = sub(result, centre)
            l2 = dot(pres, pres)
            result = centre if not l2 > 0.0 else add(centre, mul(math.sqrt(pr2 / l2), pres))
    for i in range(no):
        pp, pn = planes[i]
        if dot(pn, sub(pp, result)) > 0.0:
            cr = cross(pn, qn)
            cl2 = dot(cr, cr)
            if cl2 <= EPS:
                return None
            dirn = div(cr, math.sqrt(cl2))
            ln = cross(dirn, qn)
            s = dot(sub(pp, qp), pn) / dot(ln, pn)
            lpnt = add(qp, mul(s, ln))
            result = lp1(planes, i, dirn, lpnt, radius, opt, direction_opt)
            if result is None:
                return None
    return result


def lp3(planes, count, radius, opt, direction_opt):
    """-> (fail index or count, result, moved)"""
    if direction_opt:
        result = mul(radius, opt)
    else:
        l2 = dot(opt, opt)
        result = mul(radius, div(opt, math.sqrt(l2))) if l2 > radius * radius else opt
    moved = False
    for i in range(count):
        pp, pn = planes[i]
        if dot(pn, sub(pp, result)) > 0.0:
            moved = True
            r = lp2(planes, i, radius, opt, direction_opt)
            if r is None:
                return i, result, moved
            result = r
    return count, result, moved


def lp4(planes, count, hard, begin, radius, result):
    distance = 0.0
    for i in range(begin, count):
        ip, inn = planes[i]
        if not dot(inn, sub(ip, result)) > distance:
            continue
        proj = []
        for j in range(i):
            jp, jn = planes[j]
            if j < hard:
                proj.append((jp, jn))
                continue
            cr = cross(jn, inn)
            if dot(cr, cr) <= EPS:
                if dot(inn, jn) > 0.0:
                    continue
                point = mul(0.5, add(ip, jp))
            else:
                ln = cross(cr, inn)
                s = dot(sub(jp, ip), jn) / dot(ln, jn)
                point = add(ip, mul(s, ln))
            dn = sub(jn, inn)
            proj.append((point, unit(dn, math.sqrt(dot(dn, dn)))))
        fail, r, _ = lp3(proj, len(proj), radius, inn, True)
        if not fail < len(proj):
            result = r
        distance = dot(inn, sub(ip, result))
    return result


def solve(planes, hard, max_speed, pref):
    """-> (v, status, slack)"""
    count = len(planes)
    fail, v, moved = lp3(planes, count, max_speed, pref, False)
    if fail == count:
        return v, (2 if moved else 1), 0.0
    v = lp4(planes, count, hard, fail, max_speed, v)
    slack = 0.0
    for i in range(hard, count):
        pen = dot(planes[i][1], sub(planes[i][0], v))
        slack = pen if pen > slack else slack
    return v, 3, slack


# ---- rules 2, 3, 5 ----
def gate(p, r, b, reach, below):
    """building_pair: -> (pass, gap)"""
    ex, ey = p[0] - b[0], p[1] - b[1]
    d = math.sqrt(ex * ex + ey * ey)
    return (b[2] > p[2] - below and d <= reach), d - (r + b[3])


def planes_of(i, pos, vel, rad, n_live, buildings, vel_of, time_horizon=5.0, time_step=1.0, neighbor_dist=10.0,
              max_neighbors=10, max_buildings=4, reach=10.0, below=1.0, clear_xy=0.0, tally=None):
    """Drone i's planes in rule 5's order -> (planes, n_buildings kept).  pos, vel [N][3], rad [N], the first n_live rows
    live; buildings [nb][4]; vel_of(j) -> (vb_x, vb_y) of building j."""
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
        b = [float(x) for x in b]
        ok, gap = gate(p, r, b, reach, below)
        if ok:
            blds.append((gap, j))
    blds.sort()
    blds = blds[:max_buildings]
    out = []
    for _, j in blds:
        b = [float(x) for x in buildings[j]]
        vb = vel_of(j)
        pp, pn, br = plane((b[0] - p[0], b[1] - p[1], 0.0), (v[0] - float(vb[0]), v[1] - float(vb[1]), 0.0),
                           (r + b[3]) + clear_xy, time_horizon, time_step, 1.0, v)
        if tally is not None:
            tally["building_branch%d" % br] += 1
        out.append((pp, pn))
    for _, j in near:
        rel = (float(pos[j][0]) - p[0], float(pos[j][1]) - p[1], float(pos[j][2]) - p[2])
        w_rel = (v[0] - float(vel[j][0]), v[1] - float(vel[j][1]), v[2] - float(vel[j][2]))
        pp, pn, br = plane(rel, w_rel, r + float(rad[j]), time_horizon, time_step, 0.5, v)
        if tally is not None:
            tally["drone_branch%d" % br] += 1
        out.append((pp, pn))
    return out, len(blds)


def orca_drone(i, pos, vel, rad, n_live, des, buildings, vel_of, max_speed=2.0, pref_speed=1.0, tally=None, **kw):
    """-> dict(v, status, slack, n_neighbors, n_buildings, planes, pref)"""
    planes, kb = planes_of(i, pos, vel, rad, n_live, buildings, vel_of, tally=tally, **kw)
    pref = (pref_speed * float(des[0]), pref_speed * float(des[1]), pref_speed * float(des[2]))
    v, status, slack = solve(planes, kb, max_speed, pref)
    return dict(v=v, status=status, slack=slack, n_neighbors=len(planes) - kb, n_buildings=kb, planes=planes, pref=pref)


def orca_env(pos, vel, rad, n_live, des, buildings, vel_of=None, **kw):
    """One env: -> (out [N][3], n_neighbors, n_buildings, status [N] int32, slack [N]); rows from n_live on are zero."""
    N = len(pos)
    vel_of = vel_of or (lambda j: (0.0, 0.0))
    out, nn, nbk = np.zeros((N, 3)), np.zeros(N, np.int32), np.zeros(N, np.int32)
    status, slack = np.zeros(N, np.int32), np.zeros(N)
    for i in range(n_live):
        r = orca_drone(i, pos, vel, rad, n_live, des[i], buildings, vel_of, **kw)
        out[i], nn[i], nbk[i], status[i], slack[i] = r["v"], r["n_neighbors"], r["n_buildings"], r["status"], r["slack"]
    return out, nn, nbk, status, slack


# ---- rvo3d_vel_command ----
def vel_command(v, yaw, pitch, w, clip=True):
    """-> ([a0, a1, a2], clipped bits); clip=False: the values before clipping, bits 0"""
    wx, wy, wz = (float(x) for x in w)
    vx, vy, vz = (float(x) for x in v)
    wn = math.sqrt((wx * wx + wy * wy) + wz * wz)
    vn = math.sqrt((vx * vx + vy * vy) + vz * vz)
    r = [wn - vn, 0.0, 0.0]
    if wn > 0.0:
        turn = math.atan2(wy, wx) * RAD2DEG - float(yaw)
        r[1] = (turn - 360.0 * math.floor((turn + 180.0) / 360.0)) / 90.0
        s = wz / wn
        s = -1.0 if s < -1.0 else (1.0 if s > 1.0 else s)
        r[2] = (math.asin(s) * RAD2DEG - float(pitch)) / 90.0
    bits = 0
    for k in range(3 if clip else 0):
        if r[k] > 1.0:
            r[k], bits = 1.0, bits | (1 << k)
        elif r[k] < -1.0:
            r[k], bits = -1.0, bits | (1 << k)
    return r, bits
