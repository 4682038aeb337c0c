"""Worlds whose drone pairs sit on the decision surfaces the float32 pair filters may pre-empt (stage G and stage X1,
csrc/rvo3d_pairs.hpp), at the places where the float32 rounding of a map is largest.  CPU only: numpy and the oracle.

A pair is (i, j): `i` is the drone whose VO row the constructed decision switches on or off, `j` its partner.  The
quantity that decides - a distance, v_i . rel, the angle between rel and w - is put on BOTH sides of its exact surface,
at a distance drawn log-uniformly from about [1e-8, 1e-3]: firm for the oracle (margin >= 1e-9, the parity tests'
KNIFE) and far inside what float32 can resolve on centred coordinates of hundreds or thousands of metres.

  gate      |rel| = 10 -+ d                          row of i exists on the near side          (stage G)
  touch     |rel| = r_i + r_j -+ d (env_train)       done on the near side, row of i beyond    (stage G touch word, X1)
  touch_eval|rel| = r_i + r_j - 0.2 -+ d, receding   done on the near side                     (env_train off)
  domain    |rel| = r_i + r_j -+ d, approaching      "math domain error" on the near side, row of i beyond
  approach  v_i . rel = +-eps, |v_i|_1 about 1 / 10  row of i exists when positive; v_i = 0 exactly, 2e-9 and 1e-12
  cone      beta = tie -+ m, alpha just above the same centi-radian tie: the row exists when beta rounds below alpha;
            pairs 6 - 10 m apart, pairs just outside touching, pairs whose d^2 - R^2 straddles x1_gap
  cmax      gate pairs with one centred coordinate of i at cmax (1 - 1e-6) in even envs and cmax (1 + 1e-6) in odd ones
            (every other round the odd envs' pairs sit near the corners of the cube of 3.9 cmax, each coordinate
            placed so that float32 rounding stretches the distance: beyond what the bands allow for)
  reset     two steps: the partner waits outside the map, is reset by the first (auto-resetting) step to a start
            waypoint 10 -+ d or r_i + r_j +- d from where i has flown to (regate_resets brings the stage-G words on
            file up to date), and the second step's reward sweep - which reads those words - flags i on one side only

Everything else about a pair is arranged so that the row of i exists exactly on one side: the partner closes at 7 m/s
(t < 2), w points along rel, a small lateral velocity keeps |cos| away from 1.  j never has a row (rel . w < 0 for it).

A round is one set_state followed by observe() (the geometry is the state, actions are zero) or by step() (the
decisions are taken on the state AFTER the move: the oracle is stepped once on a scratch copy to learn every drone's
velocity after the move - which does not depend on where it starts - and the starts are put that far back).
Pairs sit on a lattice of sites, 36 m (observe) or 50 m (step) apart, around the far corner of the map, the near corner,
or outside the map but inside cmax; drones without a site rest at their start waypoints in a block at the map's centre,
where a reset sends everybody too.  Ring slots: random owners and offsets, with the offsets around the 32-offset word
boundaries, the largest offset and pairs across the ring's seam forced in.
"""
import numpy as np

import oracle as orc

MAPS = {"m20": (20.0, 20.0, 8.0), "m500": (500.0, 500.0, 10.0), "m4000": (4000.0, 4000.0, 40.0),
        "m6000x300": (6000.0, 300.0, 30.0), "m1e6": (1e6, 1e6, 100.0)}
CONTROL = "m20"  # the control: its float32 noise is a hundred times smaller
# name: (N, E, drone counts or None, the step_autoreset instantiation with {t} = env_train)
SHAPES = {"8x16": (8, 16, None, "env_kernel<2, 1, 0, {t}, false>"),
          "24x6": (24, 6, None, "env_kernel<2, 1, 32, {t}, true>"),
          "64x4": (64, 4, None, "env_kernel<2, 1, 64, {t}, false>"),
          "100x3": (100, 3, None, "env_kernel<2, 2, 128, {t}, true>"),
          "256x2": (256, 2, None, "env_kernel<2, 4, 256, {t}, true>"),
          "300x2": (300, 2, None, "env_kernel<2, 8, 0, {t}, false>"),
          "counted48x5": (48, 5, (48, 30, 40, 22, 34), "env_kernel_counted<2, 1, 64, {t}>")}
# config: env_train, per-drone radii and priorities, (mode, bucket) rounds
CONFIGS = {"train": (True, False, [("observe", "gate"), ("observe", "approach"), ("observe", "cone"), ("observe", "cmax"),
                                   ("step", "gate"), ("step", "touch"), ("step", "approach"), ("step", "cone")]),
           "radii": (True, True, [("step", "touch"), ("observe", "cone")]),
           "eval": (False, False, [("step", "touch_eval"), ("step", "domain")]),
           "reset": (True, False, [("reset", "reset")])}
NM = 3
EXP_RADIUS = 0.2
PER_SIDE = 40  # pairs a (config, mode, bucket) must put on each side of its surface


def bands(map_size):
    """cmax and x1_gap as filter_bands() (csrc/rvo3d_host_setup.hpp) derives them."""
    mx = max(map_size)
    cmax = 0.75 * mx + 16.0
    u = 2.0 ** -24
    eD = u * (2.0 * cmax + 21.0)
    band = 2.0 * (2.0 * 1.7320508 * 10.5 * eD + 3.0 * eD * eD + 8.0 * u * 110.25)
    return float(np.float32(cmax)), float(np.float32(512.0 * band))


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _dot(a, b):
    return np.sum(a * b, axis=-1, keepdims=True)


def _logu(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def _frames(rng, n, zmax):
    """Random orthonormal frames (u, t, b) with |u_z| <= zmax."""
    uz = rng.uniform(-zmax, zmax, n)
    az = rng.uniform(0.0, 2.0 * np.pi, n)
    s = np.sqrt(1.0 - uz * uz)
    u = np.stack([s * np.cos(az), s * np.sin(az), uz], axis=-1)
    t = _unit(np.cross(u, _unit(rng.normal(size=(n, 3)))))
    return u, t, np.cross(u, t)


def _match(rng, n_live, n_pairs):
    """n_pairs disjoint pairs of the ring slots 0 .. n_live-1 as (owner d, neighbour d + k mod n_live): forced offsets
    first - 1, the word boundaries 31 / 32 / 33 ..., the largest - each once with an owner just below the seam
    (d + k wraps) where one is free, then a random matching of what is left."""
    H = n_live // 2
    forced = [k for k in (1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, H - 1, H) if 1 <= k <= H]
    rng.shuffle(forced)
    free = np.ones(n_live, bool)
    out = []
    for k in forced:
        if len(out) >= n_pairs:
            break
        cand = [(n_live - 1 - s) % n_live for s in range(min(k, 4))] + list(rng.permutation(n_live)[:8])
        for d in cand:
            j = (d + k) % n_live
            if d != j and free[d] and free[j]:
                free[d] = free[j] = False
                out.append((int(d), int(j)))
                break
    rest = rng.permutation(np.flatnonzero(free))
    for a, b in zip(rest[0::2], rest[1::2]):
        if len(out) >= n_pairs:
            break
        out.append((int(a), int(b)))
    out = np.array(out, dtype=np.int64).reshape(-1, 2)
    swap = rng.random(len(out)) < 0.5  # which end is `i`
    out[swap] = out[swap][:, ::-1]
    return out


class RefBatch:
    """The oracle for a batch with or without per-env drone counts: one OracleEnv, or one per env holding that env's
    live drones; the rows of ghosts read as the zeros the device writes there, with an infinite margin."""

    def __init__(self, case, threads=4):
        self.E, self.N, self.counts = case.E, case.N, case.counts
        kw = dict(nm=NM, env_train=case.env_train, threads=threads)
        if self.counts is None:
            self.refs = [orc.OracleEnv(case.waypoints, case.n_points, case.map_size, None, radius=case.radius,
                                       priority=case.priority, **kw)]
            self.rows = [(slice(None), slice(None))]
        else:
            self.refs, self.rows = [], []
            for e, c in enumerate(self.counts):
                sub = lambda a: None if a is None else np.ascontiguousarray(a[e:e + 1, :c])
                self.refs.append(orc.OracleEnv(sub(case.waypoints), sub(case.n_points), case.map_size, None,
                                               radius=sub(case.radius), priority=sub(case.priority), **kw))
                self.rows.append((slice(e, e + 1), slice(0, int(c))))

    def _gather(self, outs, fills):
        res = []
        for k, fill in enumerate(fills):
            first = outs[0][k]
            full = np.full((self.E, self.N) + first.shape[2:], fill, dtype=first.dtype)
            for o, (es, ns) in zip(outs, self.rows):
                full[es, ns] = o[k]
            res.append(full)
        return res

    def set_state(self, **kw):
        for r, (es, ns) in zip(self.refs, self.rows):
            r.set_state(**{k: np.ascontiguousarray(np.asarray(v)[es, ns]) for k, v in kw.items()})

    def get_state(self):
        outs = [tuple(r.get_state()[k] for k in orc.STATE_FIELDS) for r in self.refs]
        return dict(zip(orc.STATE_FIELDS, self._gather(outs, [0] * len(orc.STATE_FIELDS))))

    def observe(self):
        return self._gather([r.observe() for r in self.refs], [0, 0])

    def step(self, actions, autoreset):
        a = np.asarray(actions, dtype=np.float64)
        if autoreset:
            outs = [r.step_autoreset(np.ascontiguousarray(a[es, ns])) for r, (es, ns) in zip(self.refs, self.rows)]
            return self._gather(outs, [0] * 7)
        outs = [r.step(np.ascontiguousarray(a[es, ns])) for r, (es, ns) in zip(self.refs, self.rows)]
        return self._gather(outs, [0] * 6) + [None]

    def vo_flag(self, e, i, action):
        """Whether config_vo_inf flags drone i of env e under `action` in the state as it is."""
        if self.counts is None:
            return self.refs[0].vo_inf(e, i, action)[1]
        return self.refs[e].vo_inf(0, i, action)[1]

    def margin(self):
        return self._gather([(r.margin(),) for r in self.refs], [np.inf])[0]

    @property
    def domain_count(self):
        return sum(r.domain_count for r in self.refs)

    @property
    def nan_count(self):
        return sum(r.nan_count for r in self.refs)


class Round:
    """One set_state and the call that follows it.  Per pair (flat over the envs): env, i, j, side (True: the side on
    which the row of i exists - for touch_eval: on which nobody collides), kind; expect_rows / expect_done [E, N]: what
    the construction says the oracle must answer (expect_done: pair collisions only, drones outside the map aside)."""


class Case:
    def __init__(self, shape, map_name, config, seed=0):
        self.shape_name, self.map_name, self.config = shape, map_name, config
        self.N, self.E, counts, self.kernel = SHAPES[shape]
        self.counts = None if counts is None else np.array(counts, dtype=np.int32)
        self.map_size = np.array(MAPS[map_name], dtype=np.float64)
        self.env_train, per_drone, self.plan = CONFIGS[config]
        self.cen = 0.5 * self.map_size
        self.cmax, self.x1_gap = bands(MAPS[map_name])
        self.small = max(MAPS[map_name]) < 100.0
        self.lo = 1e-7 if max(MAPS[map_name]) > 1e5 else 1e-8  # (a double at 1e6 m resolves 1.2e-10 m)
        key = [list(SHAPES).index(shape), list(MAPS).index(map_name), list(CONFIGS).index(config), seed]
        self.rng = np.random.default_rng(key)
        E, N = self.E, self.N
        self.live = np.full(E, N, np.int32) if self.counts is None else self.counts
        # start waypoints: a block at the map's centre, 1.5 m apart, at most as tall as the map; everybody flies to
        # a point 30 m beside it
        nz = int(max(1, min(6, (self.map_size[2] - 2.0) // 1.5 + 1)))
        nxy = int(np.ceil(np.sqrt(N / nz)))
        k = np.arange(N)
        grid = np.stack([k % nxy, (k // nxy) % nxy, k // (nxy * nxy)], axis=-1).astype(np.float64)
        home = self.cen + 1.5 * (grid - 0.5 * np.array([nxy - 1, nxy - 1, nz - 1]))
        self.home = np.broadcast_to(home, (E, N, 3)).copy()
        self.waypoints = np.stack([self.home, np.broadcast_to(self.cen + np.array([3.0, 30.0, 0.0]), (E, N, 3))], axis=2)
        self.n_points = np.full((E, N), 2, np.int32)
        self.radius = self.priority = None
        if per_drone:
            self.radius = np.round(self.rng.uniform(0.15, 0.4, (E, N)), 2)
            self.priority = self.rng.choice([5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0005, 4.9995], (E, N))
        self._scratch = None
        self.rounds = []
        if config == "reset":
            if self.small:
                raise ValueError("the reset rounds need a map the pairs fit into")
            # the pairs are the case's: the partner's start waypoint is the pair's site
            env, pk, pj, site = [], [], [], []
            for e in range(E):
                st = self._sites("step", "far" if e % 2 == 0 else "near", int(self.live[e]) // 2)
                m = _match(self.rng, int(self.live[e]), len(st))
                env.append(np.full(len(m), e)); pj.append(m[:, 0]); pk.append(m[:, 1]); site.append(st[:len(m)])
            self.rp = tuple(np.concatenate(x) for x in (env, pj, pk, site))
            self.waypoints[self.rp[0], self.rp[2], 0] = self.rp[3]
            reps = max(int(np.ceil(2 * PER_SIDE * 1.25 / len(self.rp[0]))), 4)
            self.rounds = [self._reset_round(r) for r in range(reps)]
            return
        for mode, bucket in self.plan:
            ppr = self._pairs_per_round(mode, bucket)
            # (domain: half of the rounds hold one side only; per-drone priorities: two pairs in five have unequal ones)
            want = 2 * PER_SIDE * (2 if bucket == "domain" else 1) * (2.5 if per_drone else 1.25)
            reps = max(int(np.ceil(want / ppr)), 4 if mode == "step" else 3)
            for r in range(reps):
                self.rounds.append(self._round(mode, bucket, r))

    # ---- where the pairs go ----
    def _sites(self, mode, where, n):
        """Up to n site centres [k, 3]."""
        X, Y, H = self.map_size
        if self.small:
            c = np.array([(a, b, d) for a in (-18.0, 18.0) for b in (-18.0, 18.0) for d in (-18.0, 18.0)])
            return (self.cen + c)[:n]
        S = 36.0 if mode == "observe" else 50.0
        reach = self.cmax - 12.0
        if where == "out":
            nx_max = int((self.cen[0] + reach - (X + 30.0)) // S) + 1
            ny_max = int((2.0 * reach - 30.0) // S) + 1
        else:
            nx_max, ny_max = int((X - 60.0) // S) + 1, int((Y - 60.0) // S) + 1
        ny = int(min(ny_max, max(1, np.ceil(np.sqrt(n)))))
        nx = int(min(nx_max, np.ceil(n / ny)))
        ix, iy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
        ix, iy = ix.ravel(), iy.ravel()
        if where == "far":
            x, y = X - 30.0 - S * ix, Y - 30.0 - S * iy
        elif where == "near":
            x, y = 30.0 + S * ix, 30.0 + S * iy
        else:
            x, y = X + 30.0 + S * ix, self.cen[1] + reach - 15.0 - S * iy
        s = np.stack([x, y, np.full(len(ix), 0.5 * H)], axis=-1)
        clear = np.hypot(s[:, 0] - self.cen[0], s[:, 1] - self.cen[1]) >= 40.0  # (the block of start waypoints)
        return s[clear][:n]

    def _cmax_sites(self, n):
        """Sites on the six faces of the cmax cube: (centre [k, 3] with the face coordinate 0, axis [k], sign [k])."""
        per = int(min(np.ceil(n / 6.0), (0.5 * self.cmax) // 46.0 * 2 + 1))
        out, ax, sg = [], [], []
        for f in range(6):
            a, s = f % 3, 1.0 if f < 3 else -1.0
            for q in range(per):
                c = np.zeros(3)
                c[(a + 1) % 3] = 46.0 * (q - 0.5 * (per - 1))
                out.append(c); ax.append(a); sg.append(s)
        order = np.argsort(np.tile(np.arange(per), 6), kind="stable")  # every face before a face's second site
        return np.array(out)[order][:n], np.array(ax)[order][:n], np.array(sg)[order][:n]

    def _pairs_per_round(self, mode, bucket):
        tot = 0
        for e in range(self.E):
            n = int(self.live[e]) // 2
            tot += len(self._cmax_sites(n)[0]) if bucket == "cmax" else len(self._sites(mode, "far", n))
        return tot

    # ---- the oracle's own velocities after a move ----
    def _moved_velocities(self, vel, yaw, pitch, actions):
        if self._scratch is None:
            self._scratch = RefBatch(self, threads=2)
        E, N = self.E, self.N
        z = np.zeros((E, N))
        self._scratch.set_state(pos=self.home, vel=vel, yaw=yaw, pitch=pitch, real_len=z, max_dev=z, extra_len=z,
                                wp_idx=np.ones((E, N), np.int32), arrive=np.zeros((E, N), np.uint8),
                                dest=np.zeros((E, N), np.uint8))
        self._scratch.step(actions, autoreset=False)
        return self._scratch.get_state()["vel"]

    def _stretched_corner(self, rng, env, dist):
        """For every pair: centred coordinates of i [M, 3] near a corner of the cube of 3.9 cmax (the k-th pair of an env
        46 m further in along x) and rel [M, 3] of length `dist` along the diagonal towards the centre, such that
        float32 rounds every coordinate difference but one away from zero by 0.98 ulp."""
        M = len(env)
        k = np.concatenate([np.arange((env == e).sum()) for e in range(self.E)])
        sg = np.stack([np.where((k >> a) & 1, -1.0, 1.0) for a in range(3)], axis=-1)
        mag = np.full((M, 3), 3.9 * self.cmax)
        mag[:, 0] -= 46.0 * (k // 8)
        Gi = np.float32(mag).astype(np.float64)  # a float32 value
        ulp = np.spacing(np.float32(mag)).astype(np.float64)
        ci = Gi - 0.49 * ulp  # rounds up to Gi
        n = np.round(dist[:, None] / np.sqrt(3.0) / ulp + 0.98)
        dk = (n - 0.98) * ulp  # |rel_k|: the partner's coordinate Gi - n ulp + 0.49 ulp rounds down
        dz = np.sqrt(dist * dist - dk[:, 0] ** 2 - dk[:, 1] ** 2)
        # z: the partner 0.49 ulp above a float32 value, i wherever that puts it
        cjz = np.float32(mag[:, 2] - dz).astype(np.float64) + 0.49 * ulp[:, 2]
        ci[:, 2] = cjz + dz
        dk[:, 2] = dz
        return sg * ci, -sg * dk

    def _prestate(self, env, idx, v, a, heading, vel, yaw, pitch, act):
        """Fill in the state from which the action a takes the drones (env, idx) to the velocity v (the drones slower
        than 1e-8 m/s start at rest, facing `heading`: their speed after the move is their acceleration)."""
        sp = np.linalg.norm(v, axis=-1)
        mv = sp > 1e-8
        y1 = np.where(mv, np.degrees(np.arctan2(v[:, 1], v[:, 0])), np.degrees(np.arctan2(heading[:, 1], heading[:, 0])))
        p1 = np.where(mv, np.degrees(np.arcsin(np.clip(v[:, 2] / np.where(sp > 0, sp, 1.0), -1.0, 1.0))),
                      np.degrees(np.arcsin(heading[:, 2])))
        y0 = np.mod(y1 - np.clip(90.0 * a[:, 1], -90.0, 90.0), 360.0)
        p0 = p1 - np.clip(90.0 * a[:, 2], -90.0, 90.0)
        s0 = np.where(mv, sp - a[:, 0], 0.0)
        d0 = np.stack([np.cos(np.radians(p0)) * np.cos(np.radians(y0)),
                       np.cos(np.radians(p0)) * np.sin(np.radians(y0)), np.sin(np.radians(p0))], axis=-1)
        vel[env, idx] = s0[:, None] * d0
        yaw[env, idx], pitch[env, idx], act[env, idx] = y0, p0, a

    # ---- one round ----
    def _round(self, mode, bucket, r):
        rng, E, N = self.rng, self.E, self.N
        step = mode == "step"
        where = "far" if self.small else (("far", "near")[(r // 2) % 2] if step else ("far", "near", "out")[r % 3])
        inside = where != "out" and not self.small and bucket != "cmax"
        # slots and sites
        env, pi, pj, site, fax, fsg = [], [], [], [], [], []
        for e in range(E):
            n = int(self.live[e]) // 2
            if bucket == "cmax":
                s, a, g = self._cmax_sites(n)
                fax.append(a); fsg.append(g)
            else:
                s = self._sites(mode, where, n)
            m = _match(rng, int(self.live[e]), len(s))
            env.append(np.full(len(m), e)); pi.append(m[:, 0]); pj.append(m[:, 1]); site.append(s[:len(m)])
        env, pi, pj, site = np.concatenate(env), np.concatenate(pi), np.concatenate(pj), np.concatenate(site)
        M = len(env)
        ri = np.full(M, 0.2) if self.radius is None else self.radius[env, pi]
        rj = np.full(M, 0.2) if self.radius is None else self.radius[env, pj]
        qi = np.full(M, 5.0) if self.priority is None else self.priority[env, pi]
        qj = np.full(M, 5.0) if self.priority is None else self.priority[env, pj]
        R = ri + rj
        zmax = min(1.0, (0.5 * self.map_size[2] - 0.6) / 5.3) if inside else 1.0
        u, t, b = _frames(rng, M, zmax)
        side = rng.permutation(M) % 2 == 0
        if bucket == "domain" and (r // 2) % 2 == 0:
            side[:] = True  # nobody inside the shell: the error word must stay clear
        sgn = np.where(side, 1.0, -1.0)
        mgn = _logu(rng, self.lo, 1e-3, M)
        kind = np.zeros(M, np.int64)
        # actions (vectors as the VO code reads them): small, never below the 1e-5 cut
        small = lambda: rng.choice([-1.0, 1.0], (M, 3)) * rng.uniform(0.002, 0.01, (M, 3))
        ai, aj = (small(), small()) if step else (np.zeros((M, 3)), np.zeros((M, 3)))
        anchor_i = bucket == "cmax"
        if bucket == "cmax":  # the partner lies inward of the face
            fax, fsg = np.concatenate(fax), np.concatenate(fsg)
            flip = np.where(u[np.arange(M), fax] * fsg > 0, -1.0, 1.0)[:, None]
            u, b = u * flip, b * flip
        adv = None
        if bucket == "cmax" and r % 2 == 1 and self.lo < 1e-7:  # (not on the 1e6 m map: a double resolves 5e-10 m there)
            # every other round the pairs of the odd envs sit far outside, near the corners of the cube of 3.9 cmax,
            # where only the bypass keeps the bands right - with the float32 rounding of all six coordinates pushing
            # the float32 distance up: x and y of both ends 0.49 ulp from a float32 value on the side that stretches
            # their difference, z of the partner too, rel along the cube's diagonal (see _stretched_corner)
            far_out = (env % 2) == 1
            adv, relc = self._stretched_corner(rng, env, np.where(side, 10.0 - mgn, 10.0 + mgn))
            uc = _unit(relc)
            u = np.where(far_out[:, None], uc, u)
            t = _unit(np.cross(u, _unit(rng.normal(size=(M, 3)))))
            b = np.cross(u, t)
        if bucket in ("gate", "cmax", "touch", "domain", "touch_eval"):
            surf = 10.0 if bucket in ("gate", "cmax") else (R - EXP_RADIUS if bucket == "touch_eval" else R)
            # near side: in range / touching / inside the shell
            near = side if bucket in ("gate", "cmax") else ~side
            d = surf - np.where(near, 1.0, -1.0) * mgn
            if bucket == "touch_eval":
                vi, vj = -0.5 * u + 0.02 * t, 0.7 * u + 0.04 * t
            else:
                vi, vj = 0.5 * u + 0.02 * t, -7.0 * u + 0.04 * t
            rel0 = d[:, None] * u
            if adv is not None:
                rel0 = np.where(far_out[:, None], relc, rel0)
            prm = dict(d=d)
        elif bucket == "approach":
            d = rng.uniform(5.0, 9.0, M)
            vmag = np.where(rng.random(M) < 0.5, 1.0, 10.0) * rng.uniform(0.6, 1.0, M)
            vi = vmag[:, None] * t
            vj = -7.0 * u - vi + 0.04 * b
            # three pairs per round with v_i exactly zero, two with 2e-9 m/s and one with 1e-12 m/s along rel
            kind[:min(M, 6)] = np.array([1, 1, 1, 2, 2, 3])[:min(M, 6)]
            spd = np.select([kind == 1, kind == 2, kind == 3], [0.0, 2e-9, 1e-12], 1.0)
            vi = np.where((kind > 0)[:, None], spd[:, None] * u, vi)
            vj = np.where((kind > 0)[:, None], -7.0 * u + 0.04 * b, vj)
            side = np.where(kind == 1, False, np.where(kind > 1, True, side))
            sgn = np.where(side, 1.0, -1.0)
            if step:
                ai[kind > 0, 0] = spd[kind > 0]  # from rest: the speed after the move is the acceleration
            rel0 = d[:, None] * u
            prm = dict(d=d, eps=sgn * mgn)
        elif bucket == "cone":
            kind = rng.integers(0, 3, M)  # 0: 6 - 10 m apart, 1: just outside touching, 2: d^2 - R^2 around x1_gap
            dt = np.where(kind == 0, rng.uniform(6.3, 9.7, M), R * rng.uniform(1.03, 1.3, M))
            dg = np.sqrt(R * R + self.x1_gap * rng.uniform(0.8, 1.25, M))
            okg = (kind == 2) & (dg > 1.03 * R) & (dg < 9.7)
            kind = np.where((kind == 2) & ~okg, 0, kind)
            dt = np.where(okg, dg, np.where(kind == 0, rng.uniform(6.3, 9.7, M), dt))
            ac = np.ceil(100.0 * np.arcsin(R / dt) + 0.5)  # alpha_c: the tie below it is at or above asin(R / dt)
            tie = (ac - 0.5) / 100.0
            alpha = tie + _logu(rng, 1e-6, 4e-3, M)
            d = R / np.sin(alpha)
            beta = tie - sgn * mgn
            r0 = np.cos(beta)[:, None] * u + np.sin(beta)[:, None] * t
            vi = 0.5 * r0 + 0.02 * b
            if step:
                ai = u * (rng.choice([-1.0, 1.0], M) * rng.uniform(0.003, 0.01, M))[:, None]  # along w: rv stays parallel to w
            rel0 = d[:, None] * r0
            pr = (qi / (qi + qj))[:, None]
            xi0 = site - 0.5 * rel0
            # w = (x + 2 a) - pr (2 x + v_i + v_j) = 3.5 u
            vj = ((xi0 + 2.0 * ai) - 3.5 * u) / pr - 2.0 * xi0 - vi
            prm = dict(d=d, beta=beta, pr=pr)
        else:
            raise ValueError(bucket)
        # the state that produces these velocities, and the velocities the oracle really gets from it
        pos = self.home.copy()
        vel = np.zeros((E, N, 3)); yaw = np.zeros((E, N)); pitch = np.zeros((E, N)); act = np.zeros((E, N, 3))
        if step:
            for idx, v, a in ((pi, vi, ai), (pj, vj, aj)):
                self._prestate(env, idx, v, a, u, vel, yaw, pitch, act)
            moved = self._moved_velocities(vel, yaw, pitch, act)
            vi, vj = moved[env, pi], moved[env, pj]
        else:
            vel[env, pi], vel[env, pj] = vi, vj
        # rel from the velocities as they are
        if bucket == "approach":
            gen = kind == 0
            vn = np.where(gen[:, None], vi, t)
            p = _unit(u - _dot(u, vn) * vn / _dot(vn, vn))
            rel = d[:, None] * _unit(p + (prm["eps"] / (d * _dot(vn, vn)[:, 0]))[:, None] * vn)
            rel = np.where(gen[:, None], rel, rel0)
        elif bucket == "cone":
            xi = site - 0.5 * rel0
            paa = prm["pr"] * (2.0 * xi + (vi + vj))
            w = (xi + 2.0 * ai) - paa
            wh = _unit(w)
            q = _unit(t - _dot(t, wh) * wh)
            rel = d[:, None] * (np.cos(prm["beta"])[:, None] * wh + np.sin(prm["beta"])[:, None] * q)
        else:
            rel = rel0
        if anchor_i:
            xi = self.cen + site
            f = np.where((env % 2) == 0, 1.0 - 1e-6, 1.0 + 1e-6)  # odd envs: just outside
            xi[np.arange(M), fax] = self.cen[fax] + fsg * self.cmax * f
            if adv is not None:
                xi = np.where(far_out[:, None], self.cen + adv, xi)
        else:
            xi = site - 0.5 * rel0
        xj = xi + rel
        if step:  # the starts: that far back
            pos[env, pi], pos[env, pj] = xi - vi, xj - vj
        else:
            pos[env, pi], pos[env, pj] = xi, xj
        rd = Round()
        rd.mode, rd.bucket, rd.where, rd.autoreset = mode, bucket, where, bool(step and r % 2 == 1)
        rd.pos, rd.vel, rd.yaw, rd.pitch, rd.actions = pos, vel, yaw, pitch, act
        rd.env, rd.i, rd.j, rd.side, rd.kind, rd.R = env, pi, pj, side, kind, R
        rd.xi, rd.xj, rd.vi, rd.vj, rd.ai = xi, xj, vi, vj, ai  # at decision time (after the move)
        rd.ri, rd.rj = ri, rj
        rd.prm = prm
        # pairs with unequal priorities: w depends on the absolute position and is not parallel to the relative
        # velocity, so whether a row exists is the oracle's to say (-1: nothing claimed); the filter must stand down
        rd.claim = qi == qj
        rd.expect_rows = np.zeros((E, N), np.int32)
        rd.expect_done = np.zeros((E, N), np.uint8)
        if bucket == "touch_eval":
            rd.expect_done[env[~side], pi[~side]] = rd.expect_done[env[~side], pj[~side]] = 1
        else:
            rd.expect_rows[env[side], pi[side]] = 1
            if bucket == "touch":
                rd.expect_done[env[~side], pi[~side]] = rd.expect_done[env[~side], pj[~side]] = 1
        rd.expect_rows[env[~rd.claim], pi[~rd.claim]] = rd.expect_rows[env[~rd.claim], pj[~rd.claim]] = -1
        rd.expect_domain = bool(bucket == "domain" and (~side).any())
        rd.far_envs = np.zeros(E, bool)
        if bucket == "cmax":
            rd.far_envs[np.unique(env[(env % 2) == 1])] = True
        return rd

    def _reset_round(self, r):
        rng, E, N = self.rng, self.E, self.N
        env, pj, pk, site = self.rp
        M = len(env)
        u, t, b = _frames(rng, M, min(1.0, (0.5 * self.map_size[2] - 0.6) / 10.1))
        side = rng.permutation(M) % 2 == 0  # True: i is in range of / not touching the partner: flagged
        kind = (rng.random(M) < 0.5).astype(np.int64)  # 0: gate distance, 1: touch distance
        mgn = _logu(rng, self.lo, 1e-3, M)
        R = np.full(M, 0.4)
        sgn = np.where(side, 1.0, -1.0)
        d = np.where(kind == 1, R + sgn * mgn, 10.0 - sgn * mgn)
        rel = d[:, None] * u  # from the partner's start waypoint to i
        vel = np.zeros((E, N, 3)); yaw = np.zeros((E, N)); pitch = np.zeros((E, N)); act = np.zeros((E, N, 3))
        a1 = rng.choice([-1.0, 1.0], (M, 3)) * rng.uniform(0.002, 0.01, (M, 3))
        self._prestate(env, pj, -0.3 * u + 0.01 * t, a1, u, vel, yaw, pitch, act)
        vi = self._moved_velocities(vel, yaw, pitch, act)[env, pj]
        pos = self.home.copy()
        xi = site + rel
        pos[env, pj] = xi - vi
        # the partners wait at rest in a box outside the map's near face, 3 m apart
        q = np.concatenate([np.arange((env == e).sum()) for e in range(E)])
        pos[env, pk] = np.stack([-20.0 - 3.0 * (q // 16), self.cen[1] + 3.0 * (q % 16 - 8.0),
                                 np.full(M, 0.5 * self.map_size[2])], axis=-1)
        act2 = np.zeros((E, N, 3))
        act2[env, pj] = -3.0 * u + 0.01 * b
        rd = Round()
        rd.mode, rd.bucket, rd.where, rd.autoreset = "reset", "reset", "far/near", bool(r % 2 == 1)
        rd.pos, rd.vel, rd.yaw, rd.pitch, rd.actions, rd.actions2 = pos, vel, yaw, pitch, act, act2
        rd.env, rd.i, rd.j, rd.side, rd.kind, rd.R = env, pj, pk, side, kind, R
        rd.xi, rd.xj, rd.vi = xi, site, vi
        rd.ri = rd.rj = np.full(M, 0.2)
        rd.claim = np.ones(M, bool)
        return rd

    def full_state(self, rd):
        E, N = self.E, self.N
        z = np.zeros((E, N))
        return dict(pos=rd.pos, vel=rd.vel, yaw=rd.yaw, pitch=rd.pitch, real_len=z, max_dev=z.copy(),
                    extra_len=z.copy(), wp_idx=np.ones((E, N), np.int32), arrive=np.zeros((E, N), np.uint8),
                    dest=np.zeros((E, N), np.uint8))

    def outside_map(self, p):
        return ((p < 0.0) | (p > self.map_size)).any(axis=-1)


# ---- the same decisions in float32 with no band at all ----
def _f32(x):
    return np.asarray(x, dtype=np.float32)


def _fma32(a, b, c):
    """fmaf on float32 arrays: the product is exact in double, the sum rounds once more than the device's."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _dot32(a, b):
    return _fma32(a[:, 2], b[:, 2], _fma32(a[:, 1], b[:, 1], (a[:, 0] * b[:, 0]).astype(np.float32)))


def naive_f32_side(case, rd):
    """`side` of every pair as a float32 filter WITHOUT error bands would decide it: centred coordinates cast to
    float32, fma-order sums (the arithmetic of gate_acc / x1_pairs), the threshold rounded to float32."""
    ci, cj = _f32(rd.xi - case.cen), _f32(rd.xj - case.cen)
    dl = (cj - ci).astype(np.float32)
    d2 = _dot32(dl, dl)
    rs = (_f32(rd.ri) + _f32(rd.rj)).astype(np.float32)
    b = rd.bucket
    if b == "reset":
        return np.where(rd.kind == 1, ~(d2 <= rs * rs), d2 <= np.float32(100.0))
    if b in ("gate", "cmax"):
        return d2 <= np.float32(100.0)
    if b in ("touch", "domain"):
        return ~(d2 <= rs * rs)
    if b == "touch_eval":
        th = (rs - np.float32(EXP_RADIUS)).astype(np.float32)
        return ~(d2 <= th * th)
    if b == "approach":
        return _dot32(_f32(rd.vi), dl) > np.float32(0.0)
    if b == "cone":
        pr = rd.prm["pr"]
        w = _f32((rd.xi + 2.0 * rd.ai) - pr * (2.0 * rd.xi + (rd.vi + rd.vj)))  # (w itself in double: the filter's own w is v_i + v_j)
        dp, w2 = _dot32(dl, w), _dot32(w, w)
        ct = _f32(np.cos(_tie_of(rd)))
        return (dp > 0) & (dp * dp > ((w2 * d2).astype(np.float32) * (ct * ct).astype(np.float32)))
    raise ValueError(b)


def _tie_of(rd):
    """The centi-radian tie a cone pair straddles: beta rounds below alpha exactly when beta < tie."""
    return (np.floor(100.0 * np.arcsin(rd.R / rd.prm["d"]) + 0.5) - 0.5) / 100.0
