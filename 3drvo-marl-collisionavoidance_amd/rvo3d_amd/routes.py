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

Env e of a batch draws from counter word e + env_offset: a shard whose env_offset is its first env
(sharding.shard_env_range) holds the routes the whole batch would.
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

    def _place(self, kind: int, e: int, N: int, draw: int, starts, stats):
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
            un &= ~ok
            if stats is not None:
                if t == 0:
                    stats["after0"][kind] += int(un.sum())
                stats["last_round"] = max(stats["last_round"], t)
            if not un.any():
                break
        return pos, int(un.sum())

    def sample_numpy(self, E: int, N: int, P: int, draw: int, stats: dict | None = None):
        """The rules of this module in numpy: (waypoints [E, N, P, 3] float64 - two points, then the destination -,
        n_points [E, N] int32 = 2, unplaced [E] int32).  stats (optional dict) receives `after0` = [starts, ends] still
        unplaced after round 0, `last_round` = the last round any env ran, `unplaced` = [starts, ends]."""
        if P < 2 or not 1 <= N <= 512:
            raise ValueError("need P >= 2 and 1 <= N <= 512")
        if stats is not None:
            stats.update(after0=[0, 0], last_round=0, unplaced=[0, 0])
        wp = np.empty((E, N, P, 3))
        unplaced = np.zeros(E, dtype=np.int32)
        for e in range(E):
            s, us = self._place(0, e, N, draw, None, stats)
            g, ug = self._place(1, e, N, draw, s, stats)
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

    def sample(self, E: int, N: int, P: int, draw: int, device, env_mask=None, out=None):
        """rvo3d_sample_routes: (waypoints [E, N, P, 3] float64, n_points [E, N] int32, unplaced [E] int32) on `device`,
        enqueued on torch's current stream.  env_mask [E] (bool / uint8): only those envs' rows are written.  out: the
        three tensors to write into (contiguous, of these shapes and types) instead of fresh ones."""
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
            _lib.check(_lib.lib().rvo3d_sample_routes(C.byref(cfg), E, N, P, draw & 0xFFFFFFFF,
                                                      None if m is None else C.c_void_p(m.data_ptr()),
                                                      C.c_void_p(wp.data_ptr()), C.c_void_p(npts.data_ptr()),
                                                      C.c_void_p(unp.data_ptr()), stream), "rvo3d_sample_routes")
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
