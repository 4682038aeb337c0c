"""Route re-draws: separated start / goal pairs per env from a counter-based generator, on the device
(rvo3d_sample_routes) and restated in numpy (RouteSampler.sample_numpy), bit for bit the same.

Batched counterpart of the reference's start / goal generator (uaisa_env/world/random_start_end.py: random pairs with a
minimum separation).  The result is DEFINED by the rules below, so that a wave can evaluate them in parallel:

1. Candidate(kind, e, d, t), kind 0 = start, 1 = end: the Philox4x32-10 block of counter
   (low word of env_offset + e, d, t + kind * 2^31, draw) under the key (seed low, seed high); of its words x0..x2,
   u_k = (x_k + 0.5) * 2^-32 and coord_k = rint((lo_k + u_k * (hi_k - lo_k)) * 100) / 100, every operation rounded on its
   own in float64.
2. dist2(a, b) = (dx * dx + dy * dy) + dz * dz, compared with min_sep * min_sep or min_len * min_len.
3. Placement(kind) per env: in round t = 0 .. max_tries - 1 every unplaced drone d takes c_d = Candidate(kind, e, d, t)
   and is accepted iff (a) c_d is min_sep from every point placed in an EARLIER round, (b) c_d is min_sep from the
   candidate c_j of every j < d that was unplaced at the start of the round (whether or not j is accepted), and (c) for
   ends, c_d is min_len from start_d.  A drone still unplaced after the last round keeps its last candidate.
4. Starts first, then ends; unplaced[e] counts the drones left unplaced, starts plus ends.

Drone counts (BatchedDroneEnv.set_drone_counts): RouteSampler and CityRoutePlanner draw and plan for all N lanes of an env;
set_routes takes the live rows' routes and leaves the ghosts' unused ones as they are, so a live drone's route does not
depend on its env's count.

Env e of a batch draws from counter word e + env_offset: a shard whose env_offset is its first env
(sharding.shard_env_range) holds the routes the whole batch would.

CityRoutePlanner (below) adds the buildings: rule 3 (d), which refuses a candidate inside a building's clearance
cylinder (rvo3d_sample_routes_city), and the detour planner (rvo3d_plan_routes), both restated in numpy as well.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .worlds import World

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK, _S32 = np.uint64(0xFFFFFFFF), np.uint64(32)


def philox4x32(counter, key, rounds: int = 10):
    """Philox4x32 (Salmon et al., SC'11) in numpy integer arithmetic: counter = four 32-bit words, key = two (scalars or
    arrays that broadcast).  Returns four uint32 arrays."""
    c = [np.asarray(w, dtype=np.uint64) & _MASK for w in counter]
    k = [np.asarray(w, dtype=np.uint64) & _MASK for w in key]
    for r in range(rounds):
        p0, p1 = _M0 * c[0], _M1 * c[2]  # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> _S32) ^ c[1] ^ k[0], p1 & _MASK, (p0 >> _S32) ^ c[3] ^ k[1], p0 & _MASK]
        if r + 1 < rounds:
            k = [(k[0] + _W0) & _MASK, (k[1] + _W1) & _MASK]
    return [w.astype(np.uint32) for w in np.broadcast_arrays(*c)]


class RouteSamplerConfig(C.Structure):
    """rvo3d_route_sampler (include/rvo3d.h)."""
    _fields_ = [("lo", C.c_double * 3), ("hi", C.c_double * 3), ("min_sep", C.c_double), ("min_len", C.c_double),
                ("max_tries", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64), ("env_offset", C.c_int64)]


def _dist2(a, b):
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


class RouteSampler:
    """Start / goal pairs inside [margin, size - margin] per axis (the box of synthetic_world), starts min_sep apart,
    ends min_sep apart, every route at least min_len long - where max_tries rounds suffice (see `unplaced`)."""

    def __init__(self, map_size, min_sep: float = 1.0, min_len: float = 0.0, margin: float = 1.0, max_tries: int = 32,
                 seed: int = 1234, env_offset: int = 0):
        self.map_size = np.asarray(map_size, dtype=np.float64)
        self.lo = np.full(3, float(margin))
        self.hi = self.map_size - float(margin)
        self.min_sep, self.min_len = float(min_sep), float(min_len)
        self.max_tries, self.seed, self.env_offset = int(max_tries), int(seed), int(env_offset)
        if not (np.all(np.isfinite(self.lo)) and np.all(np.isfinite(self.hi)) and np.all(self.lo < self.hi)):
            raise ValueError("the box [margin, size - margin] is empty")
        if not (self.min_sep >= 0 and self.min_len >= 0 and 1 <= self.max_tries <= 1024):
            raise ValueError("need min_sep >= 0, min_len >= 0 and max_tries in 1..1024")
        self._bufs = {}

    # -- the numpy restatement ----------------------------------------------------------
    def _candidates(self, kind: int, e: int, N: int, t: int, draw: int):
        x = philox4x32(((self.env_offset + e) & 0xFFFFFFFF, np.arange(N, dtype=np.uint64), t + (kind << 31),
                        draw & 0xFFFFFFFF), (self.seed & 0xFFFFFFFF, (self.seed >> 32) & 0xFFFFFFFF))
        u = (np.stack(x[:3], axis=-1).astype(np.float64) + 0.5) * 2.0 ** -32
        return np.rint((self.lo + u * (self.hi - self.lo)) * 100.0) / 100.0

    def _place(self, kind: int, e: int, N: int, draw: int, starts, stats, refuse=None):
        """refuse (optional): candidates [N, 3] -> [N] bool, one more reason not to accept (CityRoutePlanner's rule 3 (d))."""
        s2, l2 = self.min_sep * self.min_sep, self.min_len * self.min_len
        pos = np.zeros((N, 3))
        un = np.ones(N, dtype=bool)
        lower = np.tri(N, k=-1, dtype=bool)  # [d, j]: j < d
        for t in range(self.max_tries):
            c = self._candidates(kind, e, N, t, draw)
            pos[un] = c[un]
            near = _dist2(c[:, None, :], np.where(un[None, :, None], c[None], pos[None])) < s2  # [d, j]
            ok = ~np.any(near & np.where(un[None, :], lower, True), axis=1)
            if kind:
                ok &= _dist2(c, starts) >= l2
            if refuse is not None:
                ok &= ~refuse(c)
            un &= ~ok
            if stats is not None:
                if t == 0:
                    stats["after0"][kind] += int(un.sum())
                stats["last_round"] = max(stats["last_round"], t)
            if not un.any():
                break
        return pos, int(un.sum())

    def sample_numpy(self, E: int, N: int, P: int, draw: int, stats: dict | None = None, refuse=None):
        """The rules of this module in numpy: (waypoints [E, N, P, 3] float64 - two points, then the destination -,
        n_points [E, N] int32 = 2, unplaced [E] int32).  stats (optional dict) receives `after0` = [starts, ends] still
        unplaced after round 0, `last_round` = the last round any env ran, `unplaced` = [starts, ends].  refuse
        (optional): env index -> the `refuse` of _place for that env, or None."""
        if P < 2 or not 1 <= N <= 512:
            raise ValueError("need P >= 2 and 1 <= N <= 512")
        if stats is not None:
            stats.update(after0=[0, 0], last_round=0, unplaced=[0, 0])
        wp = np.empty((E, N, P, 3))
        unplaced = np.zeros(E, dtype=np.int32)
        for e in range(E):
            r = None if refuse is None else refuse(e)
            s, us = self._place(0, e, N, draw, None, stats, r)
            g, ug = self._place(1, e, N, draw, s, stats, r)
            wp[e, :, 0] = s
            wp[e, :, 1:] = g[:, None, :]
            unplaced[e] = us + ug
            if stats is not None:
                stats["unplaced"][0] += us
                stats["unplaced"][1] += ug
        return wp, np.full((E, N), 2, np.int32), unplaced

    def world(self, E: int, N: int, draw: int, P: int = 2, buildings=None) -> World:
        """The World of sample_numpy(E, N, P, draw): what redraw(env, draw) leaves in an env of that shape."""
        wp, npts, _ = self.sample_numpy(E, N, P, draw)
        bld = np.zeros((0, 4)) if buildings is None else np.asarray(buildings, dtype=np.float64)
        return World(wp, npts, self.map_size.copy(), bld)

    # -- the device ----------------------------------------------------------------------
    def config(self) -> RouteSamplerConfig:
        return RouteSamplerConfig((C.c_double * 3)(*self.lo), (C.c_double * 3)(*self.hi), self.min_sep, self.min_len,
                                  self.max_tries, 0, self.seed & 0xFFFFFFFFFFFFFFFF, self.env_offset)

    def sample(self, E: int, N: int, P: int, draw: int, device, env_mask=None, out=None, city=None):
        """rvo3d_sample_routes: (waypoints [E, N, P, 3] float64, n_points [E, N] int32, unplaced [E] int32) on `device`,
        enqueued on torch's current stream.  env_mask [E] (bool / uint8): only those envs' rows are written.  out: the
        three tensors to write into (contiguous, of these shapes and types) instead of fresh ones.  city (a City, see
        CityRoutePlanner.sample): rvo3d_sample_routes_city instead."""
        import torch
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:  # "cuda" -> "cuda:<current>"
            device = torch.device("cuda", torch.cuda.current_device())
        if out is None:
            out = (torch.empty((E, N, P, 3), dtype=torch.float64, device=device),
                   torch.empty((E, N), dtype=torch.int32, device=device),
                   torch.zeros((E,), dtype=torch.int32, device=device))
        wp, npts, unp = out
        want = (((E, N, P, 3), torch.float64), ((E, N), torch.int32), ((E,), torch.int32))
        for t, (shape, dt) in zip(out, want):
            if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != device:
                raise AssertionError("out must be contiguous (float64 [E,N,P,3], int32 [E,N], int32 [E]) on `device`")
        m = None
        if env_mask is not None:
            m = torch.as_tensor(env_mask, device=device).to(torch.uint8).contiguous()
            if tuple(m.shape) != (E,):
                raise AssertionError(f"env_mask must have shape ({E},)")
        cfg = self.config()
        with torch.cuda.device(device):
            stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
            tail = (E, N, P, draw & 0xFFFFFFFF, None if m is None else C.c_void_p(m.data_ptr()),
                    C.c_void_p(wp.data_ptr()), C.c_void_p(npts.data_ptr()), C.c_void_p(unp.data_ptr()), stream)
            if city is None:
                _lib.check(_lib.lib().rvo3d_sample_routes(C.byref(cfg), *tail), "rvo3d_sample_routes")
            else:
                _lib.check(_lib.lib().rvo3d_sample_routes_city(C.byref(cfg), C.byref(city), *tail),
                           "rvo3d_sample_routes_city")
        self._keep = m
        return wp, npts, unp

    def redraw(self, env, draw: int, env_mask=None):
        """New routes for `env` (a BatchedDroneEnv), or for its masked envs: sample + env.set_routes, two launches on the
        current stream, nothing read back.  The staging tensors are the sampler's own, allocated once per env shape.
        Returns them: (waypoints, n_points, unplaced)."""
        import torch
        key = (env.E, env.N, env.P, str(env.device))
        if key not in self._bufs:
            self._bufs[key] = (torch.empty((env.E, env.N, env.P, 3), dtype=torch.float64, device=env.device),
                               torch.empty((env.E, env.N), dtype=torch.int32, device=env.device),
                               torch.zeros((env.E,), dtype=torch.int32, device=env.device))
        wp, npts, unp = self.sample(env.E, env.N, env.P, draw, env.device, env_mask, out=self._bufs[key])
        env.set_routes(wp, npts, env_mask)
        return wp, npts, unp


# ---- re-draws in a city: clear sampling and the detour planner ---------------------------------------------------------

class City(C.Structure):
    """rvo3d_city (include/rvo3d.h): a host struct of device pointers."""
    _fields_ = [("buildings", C.c_void_p), ("counts", C.c_void_p), ("env_stride", C.c_int64), ("nb_max", C.c_int32),
                ("clear_xy", C.c_double), ("clear_z", C.c_double), ("pad", C.c_double)]


def _env_list(buildings, counts, e: int):
    """Env e's buildings [n, 4] float64 of a shared list [nb, 4] or of per-env sets [E or 1, nb_max, 4] with counts."""
    b = np.zeros((0, 4)) if buildings is None else np.asarray(buildings, dtype=np.float64)
    if b.ndim == 3:
        b = b[e if b.shape[0] > 1 else 0]
    b = b.reshape(-1, 4)
    return b if counts is None else b[:min(max(int(counts[e]), 0), len(b))]


class CityRoutePlanner:
    """Route re-draws that respect buildings, on the device (rvo3d_sample_routes_city, rvo3d_plan_routes) and restated in
    numpy, bit for bit the same.  include/rvo3d.h has the rules in full; in short, with R_b = r_b + clear_xy and
    top_b = h_b + clear_z for a building (x_b, y_b, h_b, r_b):

    sample: `sampler`'s rules, and a candidate is also refused while it lies inside a building of its env -
    ((p_x - x_b)^2 + (p_y - y_b)^2) < R_b^2 and p_z <= top_b; it still counts as a candidate for the drones behind it.

    plan: while a leg A -> B of the route crosses a clearance cylinder (the circle of radius R_b up to top_b), a waypoint
    is inserted beside the FIRST building it crosses: at distance R_b + pad from the axis, in the direction of the
    leg's point nearest to the axis (the leg's left normal when it runs through the axis), at the leg's height there,
    rounded to 2 decimals; the shortened leg is tested again.  A drone FAILS - keeps the points it has, is counted in
    `blocked` - when its P rows are used up, when the blocked leg is vertical, or when the new point is A or B again.

    The batched counterpart of the reference's offline preparation (uaisa_env/world/theta_star_3D.py and the hand-checked
    starts and goals), not a port of it: detours go round a building, never over it."""

    def __init__(self, sampler: RouteSampler, clear_xy: float = 0.5, clear_z: float = 0.5, pad: float = 0.25):
        self.sampler = sampler
        self.clear_xy, self.clear_z, self.pad = float(clear_xy), float(clear_z), float(pad)
        ok = all(np.isfinite(v) for v in (self.clear_xy, self.clear_z, self.pad))
        if not (ok and self.clear_xy >= 0 and self.clear_z >= 0 and self.pad > 0):
            raise ValueError("need finite clear_xy >= 0, clear_z >= 0 and pad > 0")
        self._bufs = {}

    # -- the numpy restatement ----------------------------------------------------------
    def _derived(self, bld):
        """(x, y, top, R) of a list [n, 4]."""
        return bld[:, 0], bld[:, 1], bld[:, 2] + self.clear_z, bld[:, 3] + self.clear_xy

    def inside(self, p, bld):
        """inside(p, b) for points p [..., 3] and any building b of the list bld [n, 4]: [...] bool."""
        p = np.asarray(p, dtype=np.float64)
        x, y, top, R = self._derived(np.asarray(bld, dtype=np.float64).reshape(-1, 4))
        fx, fy = p[..., 0, None] - x, p[..., 1, None] - y
        return np.any(((fx * fx + fy * fy) < R * R) & (p[..., 2, None] <= top), axis=-1)

    def sample_numpy(self, E: int, N: int, P: int, draw: int, buildings, counts=None, stats: dict | None = None):
        """RouteSampler.sample_numpy with rule 3 (d): (waypoints, n_points, unplaced)."""
        def refuse(e):
            bld = _env_list(buildings, counts, e)
            return (lambda c: self.inside(c, bld)) if len(bld) else None
        return self.sampler.sample_numpy(E, N, P, draw, stats, refuse)

    def blocks(self, A, B, bld):
        """Blocks(A, B, b) for every building of the list bld [n, 4]: (blocked [n] bool, t0 [n], tc [n]), and a."""
        x, y, top, R = self._derived(bld)
        dx, dy, dz = B[0] - A[0], B[1] - A[1], B[2] - A[2]
        a = dx * dx + dy * dy
        fx, fy = A[0] - x, A[1] - y
        c = (fx * fx + fy * fy) - R * R
        zero = np.zeros(len(bld))
        if a == 0.0:
            return (c < 0.0) & ((A[2] if A[2] < B[2] else B[2]) <= top), zero, zero, a
        bq = fx * dx + fy * dy
        disc = bq * bq - a * c
        hit = disc > 0.0
        s = np.sqrt(np.where(hit, disc, 0.0))
        t0, t1 = (-bq - s) / a, (-bq + s) / a
        hit &= ~((t1 <= 0.0) | (t0 >= 1.0))
        t0 = np.where(t0 > 0.0, t0, 0.0)
        t1 = np.where(t1 < 1.0, t1, 1.0)
        z0, z1 = A[2] + t0 * dz, A[2] + t1 * dz
        hit &= np.where(z0 < z1, z0, z1) <= top
        tc = -bq / a
        tc = np.where(tc > 0.0, tc, 0.0)
        tc = np.where(tc < 1.0, tc, 1.0)
        return hit, t0, tc, a

    def _plan_one(self, start, goal, P: int, bld):
        """Plan of include/rvo3d.h for one drone: (points, failed)."""
        pts, i = [np.array(start, dtype=np.float64), np.array(goal, dtype=np.float64)], 0
        r2 = lambda v: np.rint(v * 100.0) / 100.0
        while i < len(pts) - 1 and len(bld):
            A, B = pts[i], pts[i + 1]
            hit, t0, tcs, a = self.blocks(A, B, bld)
            idx = np.flatnonzero(hit)
            if not len(idx):
                i += 1
                continue
            b = idx[np.argmin(t0[idx])]  # the first occurrence of the minimum: the lowest index among equals
            if len(pts) == P or a == 0.0:
                return pts, True
            tc, xb, yb = tcs[b], bld[b, 0], bld[b, 1]
            dx, dy, dz = B[0] - A[0], B[1] - A[1], B[2] - A[2]
            l2 = np.sqrt(a)
            nx, ny = (A[0] + tc * dx) - xb, (A[1] + tc * dy) - yb
            nl = np.sqrt(nx * nx + ny * ny)
            if nl < 1e-6:
                nx, ny, nl = -dy, dx, l2
            D = (bld[b, 3] + self.clear_xy) + self.pad
            W = np.array([r2(xb + (nx / nl) * D), r2(yb + (ny / nl) * D), r2(A[2] + tc * dz)])
            if np.all(W == A) or np.all(W == B):
                return pts, True
            pts.insert(i + 1, W)
        return pts, False

    def plan_numpy(self, waypoints, buildings, counts=None):
        """rvo3d_plan_routes in numpy: rows 0 and 1 of waypoints [E, N, P, 3] are each drone's start and goal.  Returns
        (waypoints - a new array -, n_points [E, N] int32, blocked [E] int32, blocked_mask [E, N] uint8)."""
        src = np.asarray(waypoints, dtype=np.float64)
        E, N, P, _ = src.shape
        if P < 2 or not 1 <= N <= 512:
            raise ValueError("need P >= 2 and 1 <= N <= 512")
        wp = np.empty_like(src)
        npts = np.empty((E, N), dtype=np.int32)
        mask = np.zeros((E, N), dtype=np.uint8)
        for e in range(E):
            bld = _env_list(buildings, counts, e)
            for d in range(N):
                pts, failed = self._plan_one(src[e, d, 0], src[e, d, 1], P, bld)
                wp[e, d, :len(pts)] = pts
                wp[e, d, len(pts):] = pts[-1]
                npts[e, d], mask[e, d] = len(pts), failed
        return wp, npts, mask.sum(axis=1, dtype=np.int32), mask

    def world(self, E: int, N: int, draw: int, P: int, buildings, counts=None) -> World:
        """The World a re-draw leaves: sample_numpy, then plan_numpy, with the city they went round."""
        wp, _, _ = self.sample_numpy(E, N, P, draw, buildings, counts)
        wp, npts, _, _ = self.plan_numpy(wp, buildings, counts)
        bld = np.zeros((0, 4)) if buildings is None else np.asarray(buildings, dtype=np.float64)
        cnt = None if counts is None or bld.ndim != 3 else np.asarray(counts, dtype=np.int32)
        return World(wp, npts, self.sampler.map_size.copy(), bld, cnt)

    # -- the device ----------------------------------------------------------------------
    def _city(self, E: int, buildings, counts, device):
        """(City, the tensors it points into): buildings [nb, 4] / [1 or E, nb_max, 4], counts [E] or None - device
        tensors, or numpy, which is uploaded."""
        import torch
        dev = lambda a, dt: (a if torch.is_tensor(a) else torch.as_tensor(np.ascontiguousarray(a))).to(
            device=device, dtype=dt).contiguous()
        b = dev(np.zeros((1, 0, 4)) if buildings is None else buildings, torch.float64)
        if b.dim() == 2:
            b = b[None]
        if b.dim() != 3 or b.shape[0] not in (1, E) or b.shape[2] != 4:
            raise AssertionError(f"buildings must have shape (nb, 4), (1, nb_max, 4) or ({E}, nb_max, 4)")
        c = None if counts is None else dev(counts, torch.int32)
        if c is not None and tuple(c.shape) != (E,):
            raise AssertionError(f"counts must have shape ({E},)")
        nb_max = int(b.shape[1])
        city = City(b.data_ptr() if nb_max else None, None if c is None else c.data_ptr(),
                    0 if b.shape[0] == 1 else nb_max * 4, nb_max, self.clear_xy, self.clear_z, self.pad)
        return city, (b, c)

    def sample(self, E: int, N: int, P: int, draw: int, device, buildings, counts=None, env_mask=None, out=None):
        """rvo3d_sample_routes_city on torch's current stream: RouteSampler.sample's arguments and results, and the city."""
        import torch
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        city, self._keep_city = self._city(E, buildings, counts, device)
        return self.sampler.sample(E, N, P, draw, device, env_mask, out, city=city)

    def plan(self, waypoints, buildings, counts=None, env_mask=None, out=None):
        """rvo3d_plan_routes on torch's current stream: waypoints (a contiguous float64 device tensor [E, N, P, 3], start
        and goal in rows 0 and 1) is planned IN PLACE.  Returns (waypoints, n_points [E, N] int32, blocked [E] int32,
        blocked_mask [E, N] uint8); out: the last three, to write into instead of fresh tensors.  env_mask [E]: nothing of
        the other envs is read or written."""
        import torch
        wp = waypoints
        if not (torch.is_tensor(wp) and wp.dtype == torch.float64 and wp.dim() == 4 and wp.shape[3] == 3
                and wp.is_contiguous() and wp.is_cuda):
            raise AssertionError("waypoints must be a contiguous float64 device tensor [E, N, P, 3]")
        E, N, P, _ = wp.shape
        device = wp.device
        if out is None:
            out = (torch.empty((E, N), dtype=torch.int32, device=device), torch.zeros((E,), dtype=torch.int32, device=device),
                   torch.zeros((E, N), dtype=torch.uint8, device=device))
        want = (((E, N), torch.int32), ((E,), torch.int32), ((E, N), torch.uint8))
        for t, (shape, dt) in zip(out, want):
            if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != device:
                raise AssertionError("out must be contiguous (int32 [E,N], int32 [E], uint8 [E,N]) on the waypoints' device")
        npts, blocked, bmask = out
        m = None
        if env_mask is not None:
            m = torch.as_tensor(env_mask, device=device).to(torch.uint8).contiguous()
            if tuple(m.shape) != (E,):
                raise AssertionError(f"env_mask must have shape ({E},)")
        city, keep = self._city(E, buildings, counts, device)
        with torch.cuda.device(device):
            stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
            _lib.check(_lib.lib().rvo3d_plan_routes(C.byref(city), E, N, P, None if m is None else C.c_void_p(m.data_ptr()),
                                                    C.c_void_p(wp.data_ptr()), C.c_void_p(npts.data_ptr()),
                                                    C.c_void_p(blocked.data_ptr()), C.c_void_p(bmask.data_ptr()), stream),
                       "rvo3d_plan_routes")
        self._keep_plan = (m, keep)  # the borrowed buffers live until the launch ran
        return wp, npts, blocked, bmask

    def redraw(self, env, draw: int, env_mask=None):
        """New routes for `env` (a BatchedDroneEnv), or for its masked envs, round the city the env collides with now
        (env.device_buildings()): sample + plan + env.set_routes, three launches on the current stream, nothing read
        back.  The staging tensors are the planner's own, allocated once per env shape.  Returns (waypoints, n_points,
        unplaced, blocked); blocked_mask of the last call is `last_blocked_mask`."""
        import torch
        key = (env.E, env.N, env.P, str(env.device))
        if key not in self._bufs:
            E, N, dev = env.E, env.N, env.device
            self._bufs[key] = (torch.empty((E, N, env.P, 3), dtype=torch.float64, device=dev),
                               torch.empty((E, N), dtype=torch.int32, device=dev),
                               torch.zeros((E,), dtype=torch.int32, device=dev),
                               torch.zeros((E,), dtype=torch.int32, device=dev),
                               torch.zeros((E, N), dtype=torch.uint8, device=dev))
        wp, npts, unp, blocked, bmask = self._bufs[key]
        bld, cnt = env.device_buildings()
        self.sample(env.E, env.N, env.P, draw, env.device, bld, cnt, env_mask, out=(wp, npts, unp))
        self.plan(wp, bld, cnt, env_mask, out=(npts, blocked, bmask))
        env.set_routes(wp, npts, env_mask)
        self.last_blocked_mask = bmask
        return wp, npts, unp, blocked
