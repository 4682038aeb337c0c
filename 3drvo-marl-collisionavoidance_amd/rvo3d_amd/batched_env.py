"""BatchedDroneEnv: E environments x N drones stepped by one HIP launch.

Thin host object over the C-ABI (include/rvo3d.h).  Tensors live on the GPU
(PyTorch-ROCm is only the allocator / stream provider); every call enqueues on
torch's current stream and returns without synchronising.

Batched counterpart of the reference façade `mdin` (mdin.py:7-48):
    drone_step      -> step(actions)            (mdin.py:19-30)
    drone_reset     -> reset() ; observe()      (mdin.py:38, ir_gym.py:360)
    drone_reset_one -> reset_drones(mask)       (mdin.py:43)
    ir_gym.env_observation -> observe()         (ir_gym.py:372)
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .worlds import World

_F64 = {"pos": 3, "vel": 3, "yaw": 0, "pitch": 0, "real_len": 0, "max_dev": 0, "extra_len": 0}


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class BatchedDroneEnv:
    def __init__(self, world: World, neighbors_num: int = 10, env_train: bool = True,
                 device="cuda:0", action_decimals: int = -1, radius=None, priority=None,
                 acceler: float = 0.5, reward_f64: bool = False, reuse_obs: bool = True):
        """reuse_obs: a step into the env's own obs / vo_count leaves out the stores of the zeros the buffer
        already holds, as long as the pair is what the library last wrote there (see `step`); False makes
        every step write every byte."""
        if not torch.cuda.is_available():
            raise RuntimeError("rvo3d_amd needs a GPU: there is no CPU fallback "
                               "(the CPU oracle under oracle/ is test infrastructure only)")
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:  # "cuda" -> "cuda:<current>"
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.E, self.N, self.P = world.shape
        self.nm = int(neighbors_num)
        self.W = 12 + 9 * self.nm
        self.acceler = acceler  # ir_gym.acceler (ir_gym.py:34), used by the trainer glue
        self.env_train = bool(env_train)  # rvo_inter.env_train (rvo_inter.py:14)
        self.world = world
        L = _lib.lib()
        # a set per env (World.buildings [E, nb_max, 4]): no shared list, the sets are attached after the world is loaded
        per_env = world.per_env_buildings
        cfg = _lib.Config(self.E, self.N, self.P, 0 if per_env else int(world.buildings.shape[0]), self.nm,
                          int(bool(env_train)), self.device.index or 0, int(action_decimals),
                          (C.c_double * 3)(*[float(x) for x in world.map_size]))
        h = C.c_void_p()
        _lib.check(L.rvo3d_create(C.byref(cfg), C.byref(h)), "rvo3d_create")
        self._h = h
        self._env_bld = None  # the last set_env_buildings: (buildings, counts) host arrays, None: the world's shared list
        self._dev_bld = None  # device_buildings()' cache
        self._motion = None   # attach_building_motion: advanced in front of every step
        wp = np.ascontiguousarray(world.waypoints, dtype=np.float64)
        npts = np.ascontiguousarray(world.n_points, dtype=np.int32)
        bld = np.zeros((0, 4)) if per_env else np.ascontiguousarray(world.buildings, dtype=np.float64)
        rad = None if radius is None else np.ascontiguousarray(
            np.broadcast_to(np.asarray(radius, dtype=np.float64), (self.E, self.N)))
        pri = None if priority is None else np.ascontiguousarray(
            np.broadcast_to(np.asarray(priority, dtype=np.float64), (self.E, self.N)))
        hp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
        with torch.cuda.device(self.device):
            _lib.check(L.rvo3d_load_world(h, hp(wp), hp(npts), hp(bld) if bld.size else None,
                                          hp(rad), hp(pri), self._stream()), "rvo3d_load_world")
        if per_env:
            self.set_env_buildings(world.buildings, world.building_counts)
        E, N, dev = self.E, self.N, self.device
        self.obs = torch.zeros((E, N, self.W), dtype=torch.float32, device=dev)
        self.vo_count = torch.zeros((E, N), dtype=torch.int32, device=dev)
        self.reward = torch.zeros((E, N), dtype=torch.float32, device=dev)
        self.done = torch.zeros((E, N), dtype=torch.uint8, device=dev)
        self.info = torch.zeros((E, N), dtype=torch.uint8, device=dev)
        self.finish = torch.zeros((E, N), dtype=torch.uint8, device=dev)
        self.reset_mask = torch.zeros((E, N), dtype=torch.uint8, device=dev)
        # obs / vo_count as the library last wrote them: their version counters right after that call (None: not
        # a consistent pair, the next step writes in full).  Any in-place torch op on either tensor or a view of
        # it bumps its counter; writers that bypass it (.data, DLPack, raw pointers) call invalidate_outputs().
        self.reuse_obs = bool(reuse_obs)
        self._obs_ver = None
        self._routes_set = False  # set_routes was called: the routes are part of the checkpoint
        self._args = _lib.StepArgs()
        self._args.acceler = float(acceler)
        # optional float64 copy of the reward, as the reference returns it (mdin.py:28)
        self.reward64 = None
        if reward_f64:
            self.reward64 = torch.zeros((E, N), dtype=torch.float64, device=dev)
            _lib.check(L.rvo3d_set_reward_f64(h, _ptr(self.reward64)), "rvo3d_set_reward_f64")
        # fleets of different sizes (World.drone_counts [E]): attached once the world is loaded
        self._counts = None  # host copy of the counts in force, None: every env has N drones
        self._counts_dev = self._live = None
        self._counts_version = 0  # number of set_drone_counts calls: what a captured launch sequence was made for
        if getattr(world, "drone_counts", None) is not None:
            self.set_drone_counts(world.drone_counts)

    # -- plumbing ---------------------------------------------------------------
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().rvo3d_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_env_buildings(self, buildings, counts=None):
        """A building set per env from the next step on (rvo3d_set_env_buildings): buildings [E, nb_max, 4] = x,y,h,r,
        counts [E] (env e collides with buildings[e, :counts[e]]; None: all nb_max).  Replaces the sets in force, e.g.
        to re-draw the cities between epochs; set_env_buildings(None) goes back to the world's shared list.
        Synchronises the current stream.  Detaches a building motion (attach_building_motion)."""
        self._upload_env_buildings(buildings, counts)
        if self._motion is not None:
            self._motion._unbind()
            self._motion = None

    def _upload_env_buildings(self, buildings, counts=None):
        b = c = None
        nb_max = 0
        if buildings is not None:
            b = np.ascontiguousarray(buildings, dtype=np.float64)
            if b.ndim != 3 or b.shape[0] != self.E or b.shape[2] != 4:
                raise AssertionError(f"buildings must have shape ({self.E}, nb_max, 4)")
            nb_max = int(b.shape[1])
            if counts is not None:
                c = np.ascontiguousarray(counts, dtype=np.int32)
                if c.shape != (self.E,):
                    raise AssertionError(f"counts must have shape ({self.E},)")
        hp = lambda a: None if a is None or a.size == 0 else C.c_void_p(a.ctypes.data)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().rvo3d_set_env_buildings(self._h, hp(b), hp(c), nb_max, self._stream()),
                       "rvo3d_set_env_buildings")
        self._env_bld = None if b is None or nb_max == 0 else (b.copy(), None if c is None else c.copy())
        self._dev_bld = None

    def set_drone_counts(self, counts):
        """Per-env drone counts from the next call on (rvo3d_set_drone_counts): counts [E], each 1..N; env e then has
        the live drones 0 .. counts[e]-1 and behaves as the env of a BatchedDroneEnv built with those drones alone; the
        rows beyond are ghosts whose outputs are zeros and whose inputs are ignored.  None: every env has N drones
        again.  Envs whose count changes end up in their reset state, the others are not touched - e.g. a curriculum
        that raises the counts between epochs.  Synchronises the current stream.  obs / vo_count are not touched:
        observe() afterwards."""
        c = None
        if counts is not None:
            c = np.ascontiguousarray(counts.cpu().numpy() if torch.is_tensor(counts) else counts, dtype=np.int32)
            if c.shape != (self.E,):
                raise AssertionError(f"counts must have shape ({self.E},)")
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().rvo3d_set_drone_counts(self._h, None if c is None else C.c_void_p(c.ctypes.data),
                                                         self._stream()), "rvo3d_set_drone_counts")
        self._counts = None if c is None else c.copy()
        self._counts_dev = self._live = None
        self._counts_version += 1
        self._obs_ver = None  # the rows of the envs that changed are stale: the next step writes in full

    @property
    def drone_counts(self):
        """The counts in force as a device tensor [E] int32 (a copy of the handle's), or None."""
        if self._counts is None:
            return None
        if self._counts_dev is None:
            self._counts_dev = torch.from_numpy(self._counts).to(self.device)
        return self._counts_dev

    def drone_counts_ptr(self):
        """The handle's own device array of the counts in force (rvo3d_drone_counts) as an address, None without
        counts.  Unlike the `drone_counts` tensor it stays where it is until close(): what launches that outlive a
        set_drone_counts (captured graphs) may hold."""
        ptr = C.c_void_p()
        _lib.check(_lib.lib().rvo3d_drone_counts(self._h, C.byref(ptr)), "rvo3d_drone_counts")
        return ptr.value or None

    @property
    def live(self):
        """[E, N] bool on the device: True for the drones an env has (all True without counts).  Cached."""
        if self._live is None:
            if self._counts is None:
                self._live = torch.ones((self.E, self.N), dtype=torch.bool, device=self.device)
            else:
                self._live = torch.arange(self.N, device=self.device)[None, :] < self.drone_counts[:, None]
        return self._live

    def device_buildings(self):
        """What the env collides with now, as device tensors: (buildings [1, nb, 4] - the world's shared list - or
        [E, nb_max, 4] - the sets of the last set_env_buildings - float64, counts [E] int32 or None).  Built on first
        use and kept until the next set_env_buildings; CityRoutePlanner.redraw reads the city from here.  With a building
        motion attached: the live tensor the motion's launches keep up to date (where the buildings are now) and the
        counts."""
        if self._motion is not None:
            return self._motion.buildings, self._motion._counts
        if self._dev_bld is None:
            if self._env_bld is not None:
                b, c = self._env_bld
            else:  # the shared list rvo3d_load_world took (none for a world of per-env sets)
                b = np.zeros((0, 4)) if self.world.per_env_buildings else np.asarray(self.world.buildings, np.float64)
                b, c = b.reshape(1, -1, 4), None
            self._dev_bld = (torch.from_numpy(np.ascontiguousarray(b)).to(self.device),
                             None if c is None else torch.from_numpy(c).to(self.device))
        return self._dev_bld

    def attach_building_motion(self, motion):
        """Moving buildings (rvo3d_amd.building_motion.BuildingMotion; None detaches): from the next step on every step -
        step, step_policy, the trainer's and the evaluator's - first advances the records of the per-env sets by one
        time step (one more launch: rvo3d_move_env_buildings), then steps the drones, which are tested against the
        buildings where they are now; safety(), building_rows() and device_buildings() see them there as well.  Needs
        per-env sets in force and a motion of their shape [E, nb_max]; set_env_buildings detaches it.  The records stay
        where the motion left them when it is detached."""
        if motion is None:
            if self._motion is not None:
                # the host copy of the sets follows the buildings: what device_buildings() reports from now on
                self._env_bld = (self._motion.buildings.cpu().numpy(), self._env_bld[1])
                self._dev_bld = None
                self._motion._unbind()
                self._motion = None
            return
        if self._env_bld is None:
            raise ValueError("attach_building_motion needs per-env building sets (set_env_buildings)")
        if self._motion is not None and self._motion is not motion:
            self.attach_building_motion(None)
        b, c = self._env_bld
        if motion.shape != tuple(b.shape[:2]):
            raise ValueError(f"the motion is for [E, nb_max] = {motion.shape}, the sets in force have {tuple(b.shape[:2])}")
        motion._bind(self, b, c)
        self._motion = motion

    def set_routes(self, waypoints, n_points=None, env_mask=None):
        """New routes from the next call on (rvo3d_set_routes): waypoints [E, N, P, 3] float64, n_points [E, N] int32
        (None: P everywhere), env_mask [E] bool / uint8 (None: every env) - device tensors, or numpy, which is uploaded.
        A masked env ends up as an env of a freshly built BatchedDroneEnv with these routes, every drone in its reset
        state; the other envs are not written.  An env with an n_points entry outside 2..P keeps what it had and raises
        bit 4 of error_flags().  One launch on the current stream, no synchronisation.  obs / vo_count are not
        touched: observe() afterwards."""
        def dev(a, dt, shape, name):
            if not torch.is_tensor(a):
                a = torch.as_tensor(np.ascontiguousarray(a))
            a = a.to(device=self.device, dtype=dt).contiguous()
            if tuple(a.shape) != shape:
                raise AssertionError(f"{name} must have shape {shape}")
            return a
        wp = dev(waypoints, torch.float64, (self.E, self.N, self.P, 3), "waypoints")
        if n_points is None:
            n_points = torch.full((self.E, self.N), self.P, dtype=torch.int32, device=self.device)
        npts = dev(n_points, torch.int32, (self.E, self.N), "n_points")
        m = None if env_mask is None else dev(env_mask, torch.uint8, (self.E,), "env_mask")
        _lib.check(_lib.lib().rvo3d_set_routes(self._h, _ptr(m), _ptr(wp), _ptr(npts), self._stream()),
                   "rvo3d_set_routes")
        self._keep_routes = (wp, npts, m)  # the borrowed buffers live until the launch ran
        self._routes_set = True

    def routes(self):
        """(waypoints [E, N, P, 3] float64 padded with each destination, n_points [E, N] int32): device copies of the
        routes in force (rvo3d_get_routes)."""
        wp = torch.empty((self.E, self.N, self.P, 3), dtype=torch.float64, device=self.device)
        npts = torch.empty((self.E, self.N), dtype=torch.int32, device=self.device)
        _lib.check(_lib.lib().rvo3d_get_routes(self._h, _ptr(wp), _ptr(npts), self._stream()), "rvo3d_get_routes")
        return wp, npts

    def _actions(self, actions):
        a = actions
        if not torch.is_tensor(a):
            a = torch.as_tensor(np.asarray(a), device=self.device)
        if a.device != self.device:
            a = a.to(self.device)
        if a.dtype not in (torch.float32, torch.float64):
            a = a.to(torch.float64)
        if tuple(a.shape) != (self.E, self.N, 3):
            raise AssertionError(f"actions must have shape ({self.E}, {self.N}, 3)")  # drone.py:101
        return a.contiguous(), (1 if a.dtype == torch.float64 else 0)

    # -- observation reuse -----------------------------------------------------------
    def invalidate_outputs(self):
        """The next step writes obs / vo_count in full.  Needed only after writing either tensor in a way
        torch's version counter does not see (.data, DLPack, a raw pointer, another process)."""
        self._obs_ver = None

    def _own_versions(self):
        return (self.obs._version, self.vo_count._version)

    def _touches(self, o, c):
        """(the call writes exactly the env's own pair, it writes into the memory of either of them)"""
        po, pc = o.data_ptr() == self.obs.data_ptr(), c.data_ptr() == self.vo_count.data_ptr()
        return po and pc, po or pc

    def _call_step(self, a, dt, policy, autoreset, o, c, name):
        """rvo3d_step_ex into (o, c).  Into the env's own pair it passes prev_vo_count = vo_count when the pair is
        still exactly what the library wrote (rvo3d_step_args: the zeros already there are not stored again)."""
        own, touches = self._touches(o, c)
        args = self._args
        args.actions = a.data_ptr(); args.action_dtype = dt; args.policy = policy
        args.autoreset = 1 if autoreset else 0
        args.obs = o.data_ptr(); args.vo_count = c.data_ptr()
        args.reward = self.reward.data_ptr(); args.done = self.done.data_ptr()
        args.info = self.info.data_ptr(); args.finish = self.finish.data_ptr()
        args.reset_mask = self.reset_mask.data_ptr()
        reuse = own and self.reuse_obs and self._obs_ver is not None and self._obs_ver == self._own_versions()
        args.prev_vo_count = c.data_ptr() if reuse else None
        if touches:
            self._obs_ver = None
        if self._motion is not None:
            self._motion.advance()  # the buildings move before the drones of the same step
        _lib.check(_lib.lib().rvo3d_step_ex(self._h, C.byref(args), self._stream()), name)
        if own:
            self._obs_ver = self._own_versions()
        self._last_actions = a  # keep the borrowed buffer alive until the launch ran

    # -- reference surface ----------------------------------------------------------
    def step(self, actions, autoreset: bool = False):
        """mdin.drone_step for every env.  Returns views of the handle-owned
        output tensors (obs f32 [E,N,W], vo_count, reward f32, done, info, finish)."""
        a, dt = self._actions(actions)
        self._call_step(a, dt, 0, autoreset, self.obs, self.vo_count,
                        "rvo3d_step_autoreset" if autoreset else "rvo3d_step")
        return self.obs, self.vo_count, self.reward, self.done, self.info, self.finish

    def step_policy(self, a_inc, autoreset: bool = True, obs_out=None, cnt_out=None):
        """Step from raw policy samples: the trainer's glue (multi_ppo.py:196-210,
        a = round(a_inc, 2); action = round(acceler * a + vel, 2)) runs on the device.
        a_inc: float32 [E, N, 3]."""
        a = torch.as_tensor(a_inc, device=self.device).to(torch.float32).contiguous()
        if tuple(a.shape) != (self.E, self.N, 3):
            raise AssertionError(f"a_inc must have shape ({self.E}, {self.N}, 3)")
        o, c = self._outs(obs_out, cnt_out)
        self._args.acceler = float(self.acceler)
        self._call_step(a, _lib.RVO3D_F32, 1, autoreset, o, c, "rvo3d_step_policy")
        return o, c, self.reward, self.done, self.info, self.finish

    def reset(self, env_mask=None):
        m = None
        if env_mask is not None:
            m = torch.as_tensor(env_mask, device=self.device).to(torch.uint8).contiguous()
        _lib.check(_lib.lib().rvo3d_reset(self._h, _ptr(m), self._stream()), "rvo3d_reset")
        self._keep = m

    def reset_drones(self, mask):
        m = torch.as_tensor(mask, device=self.device).to(torch.uint8).reshape(self.E, self.N)
        m = m.contiguous()
        _lib.check(_lib.lib().rvo3d_reset_drones(self._h, _ptr(m), self._stream()),
                   "rvo3d_reset_drones")
        self._keep = m

    def _outs(self, obs_out, cnt_out):
        """Observation outputs: the env's own tensors, or caller-provided ones (e.g. the next
        slot of a rollout buffer: the kernel writes there directly, nothing is copied; always in full)."""
        if obs_out is None:
            return self.obs, self.vo_count
        if (obs_out.dtype != torch.float32 or cnt_out.dtype != torch.int32 or not obs_out.is_contiguous()
                or not cnt_out.is_contiguous() or tuple(obs_out.shape) != (self.E, self.N, self.W)
                or tuple(cnt_out.shape) != (self.E, self.N) or obs_out.device != self.device):
            raise AssertionError("obs_out / cnt_out must be contiguous float32 [E,N,W] / int32 [E,N] on the env's device")
        return obs_out, cnt_out

    def observe(self, obs_out=None, cnt_out=None):
        o, c = self._outs(obs_out, cnt_out)
        own, touches = self._touches(o, c)
        if touches:
            self._obs_ver = None
        _lib.check(_lib.lib().rvo3d_observe(self._h, _ptr(o), _ptr(c), self._stream()), "rvo3d_observe")
        if own:
            self._obs_ver = self._own_versions()
        return o, c

    def observe_envs(self, env_mask):
        """observe() for the envs whose mask byte is non-zero (rvo3d_observe_envs): their rows of the env's own obs /
        vo_count are rewritten, the other envs keep the observation of their last step.  env_mask: [E] bytes / bools."""
        m = torch.as_tensor(env_mask, device=self.device).to(torch.uint8).contiguous()
        if tuple(m.shape) != (self.E,):
            raise AssertionError(f"env_mask must have shape ({self.E},)")
        if getattr(self, "_scratch", None) is None:
            self._scratch = (torch.zeros_like(self.obs), torch.zeros_like(self.vo_count))
        so, sc = self._scratch
        # rows are copied whole from a full observation: a consistent pair stays one (see _call_step)
        keep = self._obs_ver is not None and self._obs_ver == self._own_versions()
        self._obs_ver = None
        _lib.check(_lib.lib().rvo3d_observe_envs(self._h, _ptr(m), _ptr(self.obs), _ptr(self.vo_count), _ptr(so), _ptr(sc),
                                                 self._stream()), "rvo3d_observe_envs")
        if keep:
            self._obs_ver = self._own_versions()
        self._keep = m
        return self.obs, self.vo_count

    def eval_action(self, a, acceler_vel: float = 1.0):
        """The evaluator's glue (post_train.py:63-74) on the device: acceler_vel * round(a, 2) + vel in numpy's own
        types, not rounded again (rvo3d_eval_action).  a: float32 [E, N, 3].  Returns the env's persistent float64
        [E, N, 3] action buffer, overwritten by the next call."""
        a = torch.as_tensor(a, device=self.device).to(torch.float32).contiguous()
        if tuple(a.shape) != (self.E, self.N, 3):
            raise AssertionError(f"a must have shape ({self.E}, {self.N}, 3)")
        if getattr(self, "_action64", None) is None:
            self._action64 = torch.empty((self.E, self.N, 3), dtype=torch.float64, device=self.device)
        _lib.check(_lib.lib().rvo3d_eval_action(self._h, _ptr(a), float(acceler_vel), _ptr(self._action64),
                                                self._stream()), "rvo3d_eval_action")
        self._keep_a = a
        return self._action64

    def safety(self, near_margin: float = 0.5):
        """Safety metrics of the current state (rvo3d_safety_scan; the rules are in include/rvo3d.h): (sep, bclear, wall
        float64 [E, N], near_pairs int32 [E]) - per drone the gap to the nearest other drone of its env, to the
        buildings that reach up to it and to the map faces (<= 0, <= 0 and < 0: what `done` reports), per env the
        pairs within near_margin of touching.  Ghost rows are +inf.  Call it behind a plain step(): behind
        step(autoreset=True) a reset env shows its reset state.  The env's persistent tensors, overwritten by the next
        call; one launch, no synchronisation."""
        if getattr(self, "_safety", None) is None:
            f64 = dict(dtype=torch.float64, device=self.device)
            self._safety = (torch.empty((self.E, self.N), **f64), torch.empty((self.E, self.N), **f64),
                            torch.empty((self.E, self.N), **f64), torch.empty(self.E, dtype=torch.int32, device=self.device))
        s = self._safety
        _lib.check(_lib.lib().rvo3d_safety_scan(self._h, float(near_margin), _ptr(s[0]), _ptr(s[1]), _ptr(s[2]), _ptr(s[3]),
                                                self._stream()), "rvo3d_safety_scan")
        return s

    def _motion_args(self):
        """(rvo3d_building_motion or None, dt) of the motion attached now: what rvo3d_building_rows_moving takes."""
        if self._motion is None:
            return None, 0.0
        return C.byref(self._motion._args), self._motion.dt

    def building_rows(self, k: int = 4, reach: float = 5.0, below: float = 2.0, velocity: bool = False):
        """The k nearest buildings of every drone in the current state (rvo3d_building_rows; the rules are in
        include/rvo3d.h): (rows [E, N, k, 6] float32, b_count [E, N] int32).  A building counts when it passes the
        reference's gate (rvo_inter.preprocess: roof above p_z - below, centre within reach); a row is
        [dx, dy, dh, r_b, gap, urg], rounded to two decimals like the observation, rows by ascending gap, zeros from
        b_count on and in ghost rows.  velocity=True (rvo3d_building_rows_moving): rows [E, N, k, 8],
        [dx, dy, dh, r_b, gap, urg_rel, vb_x, vb_y] - the urgency at the velocity relative to the building's and the
        velocity the attached motion (attach_building_motion) gives the building on its next move, zeros without one.
        The env's persistent tensors (one pair per k and width), overwritten by the next call; one launch, no
        synchronisation."""
        k, rf = int(k), 8 if velocity else 6
        cache = self.__dict__.setdefault("_bld_rows", {})
        if (k, rf) not in cache and 1 <= k <= 8:
            cache[k, rf] = (torch.zeros((self.E, self.N, k, rf), dtype=torch.float32, device=self.device),
                            torch.zeros((self.E, self.N), dtype=torch.int32, device=self.device))
        rows, cnt = cache.get((k, rf), (None, None))
        a = _lib.BuildingRowsArgs(k, float(reach), float(below), None if rows is None else rows.data_ptr(), rf * k, 0,
                                  None if cnt is None else cnt.data_ptr(), None)
        if velocity:
            m, dt = self._motion_args()
            _lib.check(_lib.lib().rvo3d_building_rows_moving(self._h, C.byref(a), m, dt, self._stream()),
                       "rvo3d_building_rows_moving")
        else:
            _lib.check(_lib.lib().rvo3d_building_rows(self._h, C.byref(a), self._stream()), "rvo3d_building_rows")
        return rows, cnt

    def des_vel(self):
        out = torch.empty((self.E, self.N, 3), dtype=torch.float64, device=self.device)
        _lib.check(_lib.lib().rvo3d_des_vel(self._h, _ptr(out), self._stream()), "rvo3d_des_vel")
        return out

    def rvo_vel(self, vmax=(2.0, 2.0, 2.0), acceler: float = 0.5):
        """reciprocal_vel_obs.cal_vel for every drone (reciprocal_vel_obs.py:19-31, as
        intended: see include/rvo3d.h): the classical RVO velocity, [E, N, 3] float64."""
        out = torch.empty((self.E, self.N, 3), dtype=torch.float64, device=self.device)
        vm = (C.c_double * 3)(*[float(x) for x in vmax])
        _lib.check(_lib.lib().rvo3d_rvo_vel(self._h, vm, float(acceler), _ptr(out), self._stream()),
                   "rvo3d_rvo_vel")
        return out

    def rvo_vel_city(self, vmax=(2.0, 2.0, 2.0), acceler: float = 0.5, horizon: float = 5.0, reach: float = 10.0,
                     below: float = 1.0, clear_xy: float = 0.0, clear_z: float = 0.0, diagnostics: bool = False):
        """rvo_vel that also keeps clear of the buildings (rvo3d_rvo_vel_city; the rules are in include/rvo3d.h): every
        candidate velocity is swept against the cylinder of every building that passes the reference's gate
        (reciprocal_vel_obs.preprocess: centre within `reach`, roof above p_z - `below`) over `horizon`, with `clear_xy` /
        `clear_z` of extra clearance round the cylinder and over the roof; the choice is rvo_vel's among the candidates no
        building blocks, and the one that hits last when all are blocked.  horizon=5.0 is the reference's 10 m gate over
        its 2 m/s speed cap.  The buildings are the per-env sets while sets are attached, else the world's shared list;
        the motion attached now (attach_building_motion) is picked up at every call: each candidate is then taken relative
        to the velocity the building's next move will have.  Returns [E, N, 3] float64; with diagnostics=True also a dict
        of what the selection was made from: live_mask, cone_mask, blocked_mask (int64, bit c = candidate c), tc_min
        (float64), n_gated, tier (int32), [E, N] each.  One launch, no synchronisation."""
        out = torch.empty((self.E, self.N, 3), dtype=torch.float64, device=self.device)
        diag = {}
        if diagnostics:
            for name, dt_ in (("live_mask", torch.int64), ("cone_mask", torch.int64), ("blocked_mask", torch.int64),
                              ("tc_min", torch.float64), ("n_gated", torch.int32), ("tier", torch.int32)):
                diag[name] = torch.empty((self.E, self.N), dtype=dt_, device=self.device)
        a = _lib.RvoCityArgs((C.c_double * 3)(*[float(x) for x in vmax]), float(acceler), float(reach), float(below),
                             float(horizon), float(clear_xy), float(clear_z), out.data_ptr(),
                             *[diag[n].data_ptr() if diagnostics else None
                               for n in ("live_mask", "cone_mask", "blocked_mask", "tc_min", "n_gated", "tier")])
        m, dt = self._motion_args()
        _lib.check(_lib.lib().rvo3d_rvo_vel_city(self._h, C.byref(a), m, dt, self._stream()), "rvo3d_rvo_vel_city")
        return (out, diag) if diagnostics else out

    def orca_vel(self, time_horizon: float = 5.0, time_step: float = 1.0, max_speed: float = 2.0, pref_speed: float = 1.0,
                 neighbor_dist: float = 10.0, max_neighbors: int = 10, max_buildings: int = 4, reach: float = 10.0,
                 below: float = 1.0, clear_xy: float = 0.0, diagnostics: bool = False):
        """The ORCA velocity of every drone (rvo3d_orca_vel; the rules are in include/rvo3d.h): one half-space of
        permitted velocities per kept neighbour (the `max_neighbors` nearest within `neighbor_dist`, each drone taking
        half of the avoidance) and per kept building (the `max_buildings` of least gap among those that pass the gate
        `reach` / `below`, as upright cylinders of unlimited height widened by `clear_xy`, taking no share), and the
        velocity nearest pref_speed * des_vel inside them and the ball of `max_speed`, by the published linear programs.
        Collision-free for `time_horizon` when every drone flies its result - which needs velocity_command: a velocity
        handed to step() as it is is read as an action.  The buildings are the per-env sets while sets are attached, else
        the world's shared list; the motion attached now (attach_building_motion) is picked up at every call.  Returns
        [E, N, 3] float64; with diagnostics=True also a dict of n_neighbors, n_buildings, status (int32; 0 ghost, 1 the
        preferred velocity was feasible, 2 solved by the program, 3 infeasible: the fallback's least penetration) and
        slack (float64: the largest penetration of a drone plane, 0 unless status 3), [E, N] each.  One launch, no
        synchronisation, behind a first call that allocates the handle's plane workspace."""
        out = torch.empty((self.E, self.N, 3), dtype=torch.float64, device=self.device)
        diag = {}
        names = ("n_neighbors", "n_buildings", "status", "slack")
        if diagnostics:
            for name in names:
                diag[name] = torch.empty((self.E, self.N), dtype=torch.float64 if name == "slack" else torch.int32,
                                         device=self.device)
        a = _lib.OrcaArgs(float(time_horizon), float(time_step), float(max_speed), float(pref_speed), float(neighbor_dist),
                          int(max_neighbors), int(max_buildings), float(reach), float(below), float(clear_xy),
                          out.data_ptr(), *[diag[n].data_ptr() if diagnostics else None for n in names])
        m, dt = self._motion_args()
        _lib.check(_lib.lib().rvo3d_orca_vel(self._h, C.byref(a), m, dt, self._stream()), "rvo3d_orca_vel")
        return (out, diag) if diagnostics else out

    def velocity_command(self, vel, return_clipped: bool = False):
        """The action that makes the next step() fly the velocity `vel` [E, N, 3] (rvo3d_vel_command; the formulas are in
        include/rvo3d.h): speed change, yaw and pitch increments from the current velocity and heading, each clipped to
        [-1, 1] as the step would clip it.  Returns [E, N, 3] float64, with return_clipped=True also uint8 [E, N]: bit k set
        where component k was clipped (the step then does not reach `vel`).  Ghost rows are zero.
        On a handle with action_decimals >= 0 the command is quantised like any action; evaluation envs use -1.  The
        step's RVO reward and VO rows still read the action as if it were a velocity (quirk Q3): that does not matter to
        success, length, speed or the safety figures."""
        w = torch.as_tensor(vel, device=self.device).to(torch.float64).contiguous()
        if tuple(w.shape) != (self.E, self.N, 3):
            raise ValueError(f"vel must be [{self.E}, {self.N}, 3], not {tuple(w.shape)}")
        out = torch.empty((self.E, self.N, 3), dtype=torch.float64, device=self.device)
        clipped = torch.empty((self.E, self.N), dtype=torch.uint8, device=self.device) if return_clipped else None
        _lib.check(_lib.lib().rvo3d_vel_command(self._h, _ptr(w), _ptr(out), None if clipped is None else _ptr(clipped),
                                                self._stream()), "rvo3d_vel_command")
        return (out, clipped) if return_clipped else out

    def shield_action(self, action, time_horizon: float = 5.0, time_step: float = 1.0, max_speed: float = 2.0,
                      neighbor_dist: float = 10.0, max_neighbors: int = 10, max_buildings: int = 4, reach: float = 10.0,
                      below: float = 1.0, clear_xy: float = 0.0, diagnostics: bool = False, totals=None):
        """The action shield (rvo3d_shield_action; the rules are in include/rvo3d.h): ORCA as a safety filter behind any
        controller.  For every drone the velocity the next step() would fly for `action` [E, N, 3] is held against the
        ORCA planes of the current state (orca_vel's, except that a parked neighbour takes no share); where it satisfies
        them the action comes back bit for bit, where it does not it is replaced by the velocity_command for the
        permitted velocity nearest to it.  Parked drones, rows with a non-finite action and ghost rows are not judged.
        Returns [E, N, 3] float64; with diagnostics=True also a dict of pref_vel, out_vel ([E, N, 3] float64), status
        (int32, orca_vel's; 0 not judged), flags (uint8: 8 intervened, 1 / 2 / 4 the command's clipped components) and
        slack (float64), [E, N] each.  totals: an int64 [E, 4] device tensor the call adds the env's judged, intervened,
        fallback (status 3) and clipped-command rows to; the caller zeroes it.  The motion attached now is picked up at
        every call.  One launch, no synchronisation.
        Limits: a command that clips does not reach the permitted velocity; on a handle with action_decimals >= 0 the
        step quantises the action and the shield predicts the unquantised one; buildings are cylinders of unlimited
        height; the half share assumes that the other drone is shielded too."""
        a_in = torch.as_tensor(action, device=self.device).to(torch.float64).contiguous()
        if tuple(a_in.shape) != (self.E, self.N, 3):
            raise ValueError(f"action must be [{self.E}, {self.N}, 3], not {tuple(a_in.shape)}")
        if totals is not None and (totals.dtype != torch.int64 or tuple(totals.shape) != (self.E, 4)
                                   or not totals.is_contiguous() or totals.device != a_in.device):
            raise ValueError(f"totals must be a contiguous int64 [{self.E}, 4] tensor on the env's device")
        out = torch.empty((self.E, self.N, 3), dtype=torch.float64, device=self.device)
        diag = {}
        names = ("pref_vel", "out_vel", "status", "flags", "slack")
        if diagnostics:
            for name, dt_ in zip(names, (torch.float64, torch.float64, torch.int32, torch.uint8, torch.float64)):
                diag[name] = torch.empty((self.E, self.N, 3) if name.endswith("_vel") else (self.E, self.N), dtype=dt_,
                                         device=self.device)
        a = _lib.ShieldArgs(float(time_horizon), float(time_step), float(max_speed), float(neighbor_dist),
                            int(max_neighbors), int(max_buildings), float(reach), float(below), float(clear_xy),
                            a_in.data_ptr(), out.data_ptr(), *[diag[n].data_ptr() if diagnostics else None for n in names],
                            None if totals is None else totals.data_ptr())
        m, dt = self._motion_args()
        _lib.check(_lib.lib().rvo3d_shield_action(self._h, C.byref(a), m, dt, self._stream()), "rvo3d_shield_action")
        return (out, diag) if diagnostics else out

    # -- state ------------------------------------------------------------------------
    def get_state(self):
        E, N, dev = self.E, self.N, self.device
        s = {k: torch.empty((E, N, 3) if d else (E, N), dtype=torch.float64, device=dev)
             for k, d in _F64.items()}
        s["wp_idx"] = torch.empty((E, N), dtype=torch.int32, device=dev)
        s["arrive"] = torch.empty((E, N), dtype=torch.uint8, device=dev)
        s["dest"] = torch.empty((E, N), dtype=torch.uint8, device=dev)
        order = ("pos", "vel", "yaw", "pitch", "real_len", "max_dev", "extra_len", "wp_idx",
                 "arrive", "dest")
        _lib.check(_lib.lib().rvo3d_get_state(self._h, *[_ptr(s[k]) for k in order],
                                              self._stream()), "rvo3d_get_state")
        return s

    @property
    def vel(self):
        """drone_list[i].vel of every drone (the trainer's / evaluator's reach-through,
        multi_ppo.py:202, post_train.py:72): a fresh [E, N, 3] float64 copy."""
        v = torch.empty((self.E, self.N, 3), dtype=torch.float64, device=self.device)
        none = [None] * 8
        _lib.check(_lib.lib().rvo3d_get_state(self._h, None, _ptr(v), *none, self._stream()),
                   "rvo3d_get_state")
        return v

    def set_state(self, **kw):
        order = ("pos", "vel", "yaw", "pitch", "real_len", "max_dev", "extra_len", "wp_idx",
                 "arrive", "dest")
        t = {}
        for k in order:
            v = kw.get(k)
            if v is None:
                t[k] = None
                continue
            dt = torch.int32 if k == "wp_idx" else (torch.uint8 if k in ("arrive", "dest")
                                                    else torch.float64)
            t[k] = torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v,
                                   device=self.device).to(dt).contiguous()
        _lib.check(_lib.lib().rvo3d_set_state(self._h, *[_ptr(t[k]) for k in order],
                                              self._stream()), "rvo3d_set_state")
        self._keep = t

    # -- checkpoint / resume -----------------------------------------------------------
    def state_dict(self):
        """The complete mutable state of every drone (drone.py:14-82) as CPU tensors, plus the
        shape it belongs to: enough to resume a rollout bit-exactly (the values the step keeps
        on file between calls are derived data and are rebuilt by load_state_dict).  Once set_routes has been
        called the routes in force go along (`waypoints`, `n_points`); an untouched env's are its world's."""
        sd = {k: v.cpu() for k, v in self.get_state().items()}
        sd["shape"] = torch.tensor([self.E, self.N, self.P, self.nm])
        if self._routes_set:
            wp, npts = self.routes()
            sd["waypoints"], sd["n_points"] = wp.cpu(), npts.cpu()
        if self._counts is not None:
            sd["drone_counts"] = torch.from_numpy(self._counts.copy())
        return sd

    def load_state_dict(self, sd):
        shape = [int(x) for x in sd["shape"]]
        if shape != [self.E, self.N, self.P, self.nm]:
            raise ValueError(f"checkpoint is for E,N,P,nm = {shape}, this env has "
                             f"{[self.E, self.N, self.P, self.nm]}")
        # the routes on full envs (with counts attached set_routes would leave the ghosts' routes as they are, and a later
        # set_drone_counts that raises a count would fly them), then the counts: both reset drones, the state below
        # follows them
        if "waypoints" in sd:
            if self._counts is not None:
                self.set_drone_counts(None)
            self.set_routes(sd["waypoints"], sd["n_points"])
        if "drone_counts" in sd or self._counts is not None:
            self.set_drone_counts(sd.get("drone_counts"))
        self.set_state(**{k: v for k, v in sd.items() if k not in ("shape", "waypoints", "n_points", "drone_counts")})

    def error_flags(self) -> int:
        """Reads and clears the device error word (synchronises)."""
        f = C.c_uint32(0)
        _lib.check(_lib.lib().rvo3d_error_flags(self._h, C.byref(f), self._stream()),
                   "rvo3d_error_flags")
        return int(f.value)

    def check_finite(self):
        """The reference raises ValueError when an observation holds NaN/Inf
        (ir_gym.py:232-239); opt-in here because it synchronises."""
        f = self.error_flags()
        if f & 4:  # RVO3D_FLAG_BAD_ROUTE
            raise ValueError("set_routes: n_points entries must be in [2, max_points] (the env kept its routes)")
        if f & 2:  # RVO3D_FLAG_DOMAIN_ERROR: vel_obs3D.py:13 asin((r + mr) / norm), env_train=False
            raise ValueError("math domain error")
        if f & 1:
            raise ValueError("observation contains NaN/Inf")

    def kernel_name(self, mode="step_autoreset") -> str:
        """The env_kernel instantiation the library launches for `mode` (rvo3d_kernel_name)."""
        m = {"observe": 0, "step": 1, "step_autoreset": 2}[mode]
        buf = C.create_string_buffer(128)
        _lib.check(_lib.lib().rvo3d_kernel_name(self._h, m, buf, 128), "rvo3d_kernel_name")
        return buf.value.decode()

    def launch_info(self):
        v = [C.c_int32(0) for _ in range(4)]
        _lib.check(_lib.lib().rvo3d_launch_info(self._h, *[C.byref(x) for x in v]), "launch_info")
        return dict(threads=v[0].value, envs_per_block=v[1].value, blocks=v[2].value,
                    lds_bytes=v[3].value)


class BuildingObsEnv(BatchedDroneEnv):
    """A BatchedDroneEnv whose observation shows the buildings: behind the 12 proprioceptive floats every row carries
    `building_rows` rows of six floats - the nearest buildings that pass the reference's gate (rvo3d_building_rows,
    include/rvo3d.h: what ir_gym.observation_reward collects as exter_obs_building and then leaves out) - and then the
    velocity-obstacle rows as before:

        [ 12 proprio | 6 * k building | 9 * nm VO ]      W = 12 + 6k + 9 * nm, state_dim = 12 + 6k, W_dense = 12 + 9 * nm

    The policy kernels take such a row with state_dim in place of 12 (KernelPolicyStep(state_dim=...); multi_ppo and
    post_train read env.state_dim).  step / step_policy / observe / observe_envs run what the plain env runs, into a dense
    pair the env owns (which keeps the plain env's zero-store reuse), then ONE widen launch into `obs` or the caller's
    obs_out [E, N, W]; reward, done, info, finish and vo_count are the plain env's.  Nothing is allocated after the first
    call and nothing synchronises.  Behind an auto-resetting step a reset drone's building rows are those of its reset
    state (velocity 0: urg 0), like its re-observed row.

    building_velocity=True: rows of eight floats, [dx, dy, dh, r_b, gap, urg_rel, vb_x, vb_y] (rvo3d_building_rows_moving) -
    W = 12 + 8k + 9 * nm, state_dim = 12 + 8k.  Every widen launch takes the building motion attached at that moment
    (attach_building_motion), or none: attach, detach and set_env_buildings need no new env; without a motion the two
    velocity floats are zeros and urg_rel is urg."""

    def __init__(self, world, *args, building_rows: int = 4, reach: float = 5.0, below: float = 2.0,
                 building_velocity: bool = False, **kwargs):
        k = int(building_rows)
        if not 1 <= k <= 8:
            raise ValueError("building_rows must be 1..8")
        if not (np.isfinite(reach) and reach > 0 and np.isfinite(below) and below >= 0):
            raise ValueError("reach must be finite and > 0, below finite and >= 0")
        super().__init__(world, *args, **kwargs)
        self.building_k, self.reach, self.below = k, float(reach), float(below)
        self.W_dense = self.W
        self.building_velocity = bool(building_velocity)
        self.building_row_floats = 8 if self.building_velocity else 6
        self.state_dim = 12 + self.building_row_floats * k
        self.W = self.W_dense + self.building_row_floats * k
        self._dense = self.obs  # [E, N, W_dense]: what the step and the observation write; with vo_count the reuse pair
        self.obs = torch.zeros((self.E, self.N, self.W), dtype=torch.float32, device=self.device)
        self._dense_scratch = None
        self._wargs = _lib.BuildingRowsArgs(k, self.reach, self.below, None, self.W, 12, None, self._dense.data_ptr())

    # the pair the library keeps consistent is (dense, vo_count)
    def _own_versions(self):
        return (self._dense._version, self.vo_count._version)

    def _touches(self, o, c):
        po, pc = o.data_ptr() == self._dense.data_ptr(), c.data_ptr() == self.vo_count.data_ptr()
        return po and pc, po or pc

    def _widen(self, out):
        """dense + the building rows of the current state -> out [E, N, W] (rvo3d_building_rows or, with
        building_velocity, rvo3d_building_rows_moving and the motion attached now; widen mode)."""
        self._wargs.rows = out.data_ptr()
        if self.building_velocity:
            m, dt = self._motion_args()
            _lib.check(_lib.lib().rvo3d_building_rows_moving(self._h, C.byref(self._wargs), m, dt, self._stream()),
                       "rvo3d_building_rows_moving")
        else:
            _lib.check(_lib.lib().rvo3d_building_rows(self._h, C.byref(self._wargs), self._stream()), "rvo3d_building_rows")
        return out

    def step(self, actions, autoreset: bool = False):
        a, dt = self._actions(actions)
        self._call_step(a, dt, 0, autoreset, self._dense, self.vo_count,
                        "rvo3d_step_autoreset" if autoreset else "rvo3d_step")
        self._widen(self.obs)
        return self.obs, self.vo_count, self.reward, self.done, self.info, self.finish

    def step_policy(self, a_inc, autoreset: bool = True, obs_out=None, cnt_out=None):
        a = torch.as_tensor(a_inc, device=self.device).to(torch.float32).contiguous()
        if tuple(a.shape) != (self.E, self.N, 3):
            raise AssertionError(f"a_inc must have shape ({self.E}, {self.N}, 3)")
        o, c = self._outs(obs_out, cnt_out)
        self._args.acceler = float(self.acceler)
        self._call_step(a, _lib.RVO3D_F32, 1, autoreset, self._dense, c, "rvo3d_step_policy")
        self._widen(o)
        return o, c, self.reward, self.done, self.info, self.finish

    def observe(self, obs_out=None, cnt_out=None):
        o, c = self._outs(obs_out, cnt_out)
        own, touches = self._touches(self._dense, c)
        if touches:
            self._obs_ver = None
        _lib.check(_lib.lib().rvo3d_observe(self._h, _ptr(self._dense), _ptr(c), self._stream()), "rvo3d_observe")
        if own:
            self._obs_ver = self._own_versions()
        self._widen(o)
        return o, c

    def observe_envs(self, env_mask):
        """observe() for the masked envs.  Every env's row is widened again: the building rows are a function of the
        state alone, so an env that was not re-observed gets back the floats it had."""
        m = torch.as_tensor(env_mask, device=self.device).to(torch.uint8).contiguous()
        if tuple(m.shape) != (self.E,):
            raise AssertionError(f"env_mask must have shape ({self.E},)")
        if self._dense_scratch is None:
            self._dense_scratch = (torch.zeros_like(self._dense), torch.zeros_like(self.vo_count))
        so, sc = self._dense_scratch
        keep = self._obs_ver is not None and self._obs_ver == self._own_versions()
        self._obs_ver = None
        _lib.check(_lib.lib().rvo3d_observe_envs(self._h, _ptr(m), _ptr(self._dense), _ptr(self.vo_count), _ptr(so),
                                                 _ptr(sc), self._stream()), "rvo3d_observe_envs")
        if keep:
            self._obs_ver = self._own_versions()
        self._keep = m
        self._widen(self.obs)
        return self.obs, self.vo_count
