"""The three step entry points the package itself never calls (rvo3d_step, rvo3d_step_autoreset, rvo3d_step_policy)
against rvo3d_step_ex with the equivalent rvo3d_step_args: two handles on one world, the same actions, every
output and every field of the state equal bit for bit after every step.  3 envs x 5 drones: a one-wave generic
kernel with a partial workgroup; on a 12 x 12 x 5 map with buildings drones collide and leave the map within a
few steps, so the auto-reset forms hand out reset masks."""
import ctypes as C

import numpy as np
import pytest
import torch

from rvo3d_amd import BatchedDroneEnv, _lib, synthetic_actions, synthetic_world

pytestmark = pytest.mark.gpu

E, N, NM, STEPS = 3, 5, 3, 6
ACCELER = 0.5
OUTS = ("obs", "vo_count", "reward", "done", "info", "finish")


@pytest.fixture(scope="module")
def world():
    return synthetic_world(E, N, (12, 12, 5), nb=3, seed=77)


class Handle:
    """An env handle with output tensors of its own, driven through the raw C-ABI."""

    def __init__(self, world):
        self.env = BatchedDroneEnv(world, neighbors_num=NM, env_train=True, device="cuda:0")
        dev = self.env.device
        self.obs = torch.zeros((E, N, 12 + 9 * NM), dtype=torch.float32, device=dev)
        self.vo_count = torch.zeros((E, N), dtype=torch.int32, device=dev)
        self.reward = torch.zeros((E, N), dtype=torch.float32, device=dev)
        self.done, self.info, self.finish = (torch.zeros((E, N), dtype=torch.uint8, device=dev) for _ in range(3))
        self.reset_mask = torch.full((E, N), 7, dtype=torch.uint8, device=dev)  # 7: never written by the library

    def _io(self):
        return [C.c_void_p(getattr(self, k).data_ptr()) for k in OUTS]

    def _call(self, name, *args):
        stream = C.c_void_p(torch.cuda.current_stream(self.env.device).cuda_stream)
        _lib.check(getattr(_lib.lib(), name)(self.env._h, *args, stream), name)

    def legacy(self, kind, a):
        p = C.c_void_p(a.data_ptr())
        dt = _lib.RVO3D_F64 if a.dtype == torch.float64 else _lib.RVO3D_F32
        mask = C.c_void_p(self.reset_mask.data_ptr())
        if kind == "step":
            self._call("rvo3d_step", p, dt, *self._io())
        elif kind == "autoreset":
            self._call("rvo3d_step_autoreset", p, dt, *self._io(), mask)
        else:
            self._call("rvo3d_step_policy", p, C.c_float(ACCELER), *self._io(), mask, 1 if kind == "policy_reset" else 0)

    def ex(self, kind, a):
        s = _lib.StepArgs()
        s.actions = a.data_ptr()
        s.action_dtype = _lib.RVO3D_F64 if a.dtype == torch.float64 else _lib.RVO3D_F32
        s.policy = 1 if kind.startswith("policy") else 0
        s.acceler = ACCELER
        s.autoreset = 1 if kind in ("autoreset", "policy_reset") else 0
        for k in OUTS:
            setattr(s, k, getattr(self, k).data_ptr())
        s.reset_mask = self.reset_mask.data_ptr()  # (an absolute step without auto-reset must leave it alone)
        s.prev_vo_count = None
        self._call("rvo3d_step_ex", C.byref(s))

    def snapshot(self):
        torch.cuda.synchronize()
        snap = {k: getattr(self, k).cpu().numpy().copy() for k in OUTS + ("reset_mask",)}
        snap.update({"state." + k: v.cpu().numpy() for k, v in self.env.get_state().items()})
        return snap

    def close(self):
        self.env.close()


def actions(kind, t):
    if kind == "step":
        return torch.from_numpy(synthetic_actions(E, N, t)).cuda()  # float64
    if kind == "autoreset":
        return torch.from_numpy(synthetic_actions(E, N, t).astype(np.float32)).cuda()
    rng = np.random.Generator(np.random.Philox(key=4321, counter=[0, 0, 0, t]))
    return torch.from_numpy(np.round(rng.uniform(-1, 1, (E, N, 3)), 2).astype(np.float32)).cuda()


def assert_same(sa, sb, what):
    assert sa.keys() == sb.keys()
    for k in sa:
        assert sa[k].tobytes() == sb[k].tobytes(), f"{what}: {k} differs"


@pytest.mark.parametrize("kind", ["step", "autoreset", "policy", "policy_reset"])
def test_legacy_entry_point_equals_step_ex(world, kind):
    A, B = Handle(world), Handle(world)
    try:
        for t in range(STEPS):
            a = actions(kind, t)
            A.legacy(kind, a)
            B.ex(kind, a)
            sa, sb = A.snapshot(), B.snapshot()
            assert_same(sa, sb, f"{kind}, step {t}")
            if kind in ("autoreset", "policy_reset"):
                assert (sa["reset_mask"] <= 1).all(), "the reset mask was not written"
            else:  # only the fused reset protocol hands out a mask
                assert (sa["reset_mask"] == 7).all(), "a step without auto-reset wrote the reset mask"
        assert A.env.error_flags() == B.env.error_flags()
    finally:
        A.close()
        B.close()


def test_policy_mode_does_not_outlive_its_call(world):
    """Policy and absolute steps interleaved on one handle through the legacy entry points == the same calls
    through rvo3d_step_ex on another."""
    A, B = Handle(world), Handle(world)
    try:
        for t, kind in enumerate(["policy_reset", "autoreset", "policy_reset", "step", "policy"]):
            a = actions(kind, t)
            A.legacy(kind, a)
            B.ex(kind, a)
            assert_same(A.snapshot(), B.snapshot(), f"call {t} ({kind})")
    finally:
        A.close()
        B.close()
