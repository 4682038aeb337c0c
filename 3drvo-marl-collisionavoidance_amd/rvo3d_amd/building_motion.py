"""Moving buildings: the records of a BatchedDroneEnv's per-env building sets patrol between two endpoints, advanced on
the device by one launch per step (rvo3d_move_env_buildings; the rules are in include/rvo3d.h).

The model is the reference's parked dynamic obstacle (扩展/obs_circle.py: cal_des_vel_omni - full speed towards the goal -
and move_forward - state += vel * step_time; 扩展/motion_model.py: motion_omni), with a patrol where the reference's
obstacle stops at its goal: other traffic that does not cooperate.

    motion = synthetic_patrols(world, seed=3, speed=(0.3, 1.5), span=6.0)
    env.attach_building_motion(motion)        # every step now moves the buildings first, then the drones
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib


class BuildingMotion:
    """ends [E, nb_max, 2, 2] (endpoint 0 and 1 of every record, x then y), speed [E, nb_max] (metres per unit of dt; 0 or
    NaN: the building stands still), dt: the time step (1.0 = the reference's step_time, env_base.py:98).  numpy arrays or
    device tensors; held on the device together with leg [E, nb_max] uint8, the endpoint a record is approaching (1 at the
    start and after reset()).  Attach it with BatchedDroneEnv.attach_building_motion; one motion serves one env."""

    def __init__(self, ends, speed, dt: float = 1.0, device="cuda:0"):
        def dev(a):
            if torch.is_tensor(a):
                return a.to(dtype=torch.float64).contiguous()
            return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(device)
        ends, speed = dev(ends), dev(speed)
        if speed.dim() != 2 or tuple(ends.shape) != tuple(speed.shape) + (2, 2):
            raise ValueError("ends must have shape (E, nb_max, 2, 2) and speed (E, nb_max)")
        if ends.device != speed.device:
            raise ValueError("ends and speed must live on the same device")
        if not bool(torch.isfinite(ends).all()):
            raise ValueError("ends must be finite")
        dt = float(dt)
        if not (np.isfinite(dt) and dt >= 0):
            raise ValueError("dt must be finite and >= 0")
        self.ends, self.speed, self.dt = ends, speed, dt
        self.leg = torch.ones(tuple(speed.shape), dtype=torch.uint8, device=speed.device)
        self.buildings = None  # [E, nb_max, 4] float64: where the buildings are now (while attached)
        self._env = self._start = self._counts = None
        self._args = _lib.BuildingMotionArgs()

    @property
    def shape(self):
        return tuple(self.speed.shape)

    # -- attachment (BatchedDroneEnv.attach_building_motion) -----------------------------------------------------------
    def _bind(self, env, buildings, counts):
        """buildings [E, nb_max, 4] / counts [E] or None: the host arrays of the sets in force, the start positions."""
        if self._env is not None and self._env is not env:
            raise ValueError("this BuildingMotion is attached to another env")
        if self.ends.device != env.device:
            self.ends, self.speed, self.leg = (t.to(env.device) for t in (self.ends, self.speed, self.leg))
        self._env = env
        self._start = (np.array(buildings, dtype=np.float64), None if counts is None else np.array(counts, dtype=np.int32))
        self.buildings = torch.from_numpy(self._start[0].copy()).to(env.device)
        self._counts = None if counts is None else torch.from_numpy(self._start[1].copy()).to(env.device)
        self._args.ends, self._args.speed, self._args.leg = self.ends.data_ptr(), self.speed.data_ptr(), self.leg.data_ptr()

    def _unbind(self):
        self._env = self._start = self._counts = self.buildings = None

    def _attached(self):
        if self._env is None:
            raise RuntimeError("the BuildingMotion is not attached to an env (BatchedDroneEnv.attach_building_motion)")
        return self._env

    # -- the step -------------------------------------------------------------------------------------------------------
    def advance(self, env_mask=None):
        """One time step for every env, or for the envs whose mask byte is non-zero ([E] bools / bytes): one launch on the
        current stream, nothing allocated (a mask that is not a uint8 device tensor is converted), nothing synchronised.
        BatchedDroneEnv calls it in front of every step while the motion is attached."""
        env = self._attached()
        m = None
        if env_mask is not None:
            m = torch.as_tensor(env_mask, device=env.device).to(torch.uint8).contiguous()
            if tuple(m.shape) != (env.E,):
                raise AssertionError(f"env_mask must have shape ({env.E},)")
        _lib.check(_lib.lib().rvo3d_move_env_buildings(env._h, C.byref(self._args), self.dt,
                                                       None if m is None else C.c_void_p(m.data_ptr()),
                                                       C.c_void_p(self.buildings.data_ptr()), env._stream()),
                   "rvo3d_move_env_buildings")
        self._keep = m  # the borrowed buffer lives until the launch ran

    def _upload(self, positions, leg):
        env = self._attached()
        env._upload_env_buildings(positions, self._start[1])  # (synchronises; the motion stays attached)
        self.buildings.copy_(torch.from_numpy(np.ascontiguousarray(positions, dtype=np.float64)))
        self.leg.copy_(torch.as_tensor(leg, dtype=torch.uint8).reshape(self.shape))

    def reset(self):
        """The records back where they were when the motion was attached, leg = 1.  Goes through the host
        (rvo3d_set_env_buildings): synchronises."""
        self._upload(self._start[0], np.ones(self.shape, np.uint8))

    def state_dict(self):
        """Positions and leg (CPU tensors): with the ends and speeds the motion was built from, enough to resume."""
        self._attached()
        return {"buildings": self.buildings.cpu(), "leg": self.leg.cpu()}

    def load_state_dict(self, sd):
        b = np.ascontiguousarray(torch.as_tensor(sd["buildings"]).cpu().numpy(), dtype=np.float64)
        if b.shape != self.shape + (4,) or tuple(sd["leg"].shape) != self.shape:
            raise ValueError(f"checkpoint is for another shape than {self.shape}")
        self._upload(b, torch.as_tensor(sd["leg"]).cpu())


def synthetic_patrols(world, seed: int = 1234, speed=(0.3, 1.5), span: float = 6.0, dt: float = 1.0,
                      device="cuda:0") -> BuildingMotion:
    """Patrols for a world of per-env building sets: endpoint 0 of every record is the building's position, endpoint 1 a
    point within `span` metres of it (uniform over the disc, kept inside the map), the speed ~U(speed).  rng =
    Philox(seed, stream e) per env, as synthetic_world: env e's patrols do not depend on E."""
    if not world.per_env_buildings:
        raise ValueError("synthetic_patrols needs a world of per-env building sets (World.buildings [E, nb_max, 4])")
    b = np.asarray(world.buildings, dtype=np.float64)
    E, nb = b.shape[:2]
    L, Wd = float(world.map_size[0]), float(world.map_size[1])
    ends = np.empty((E, nb, 2, 2))
    spd = np.empty((E, nb))
    for e in range(E):
        rng = np.random.Generator(np.random.Philox(key=seed, counter=[0, 0, 0, e]))
        r, a = span * np.sqrt(rng.uniform(0, 1, nb)), rng.uniform(0, 2 * np.pi, nb)
        ends[e, :, 0] = b[e, :, :2]
        ends[e, :, 1, 0] = np.clip(b[e, :, 0] + r * np.cos(a), 0.0, L)
        ends[e, :, 1, 1] = np.clip(b[e, :, 1] + r * np.sin(a), 0.0, Wd)
        spd[e] = rng.uniform(speed[0], speed[1], nb)
    return BuildingMotion(ends, spd, dt, device)
