"""How a kernel policy step is launched: the ONE place that knows the entry points' names by precision, their argument
order, the scratch they share and which of its words must be zero before a launch.  The trainer's fused rollout
(multi_ppo._collect_fused) and the evaluator (post_train.load_policy) hand it an observation and the three outputs.

Kinds (what the models pack for them: mlp_ac.mlp_blob, rnn_ac.zero_vo_plan, rnn_ac.rnn_tiles_blob):
  "mlp", "mlp_x3"             the MLP(256, 256) actor-critic's whole step as one matrix-core kernel, bf16 / float32-class
                              products (rvo3d_policy_mlp_sample / rvo3d_policy_mlp_x3_sample);
  "rnn0"                      the biGRU actor-critic in three launches: rvo3d_reader_zero_features (the collapsed first
                              layer's inputs of every row, the list of the rows that have velocity-obstacle rows), the
                              collapsed layer on the MLP kernel (exact for the rows without), the listed rows one workgroup
                              each on the modules' own parameters (rvo3d_policy_rows);
  "rnn_tiles", "rnn_tiles_x3" the same with the listed rows in 32-row matrix-core tiles, grouped by their VO count on the
                              device (rvo3d_policy_rnn_tiles / rvo3d_policy_rnn_tiles_x3)."""
import ctypes as C

import torch

from .. import _lib

_MLP_NEEDS = "an MLP(256, 256) actor-critic on the env's observation width (mlp_ac.mlp_blob returns its packed weights)"
_RNN_NEEDS = ("an rnn_ac with a shared GRU / biGRU reader of hidden 64 or 256, in_dim 9, state_dim <= 16, (256, 256) ReLU "
              "heads, on a GPU, and 1..12 VO slots")
# kind -> (precision of the model's plans, the MLP kernel, the kernel of the listed rows, what the model has to be)
_KINDS = {
    "mlp": ("bf16", "rvo3d_policy_mlp_sample", None, _MLP_NEEDS),
    "mlp_x3": ("x3", "rvo3d_policy_mlp_x3_sample", None, _MLP_NEEDS),
    "rnn0": ("bf16", "rvo3d_policy_mlp_sample", "rvo3d_policy_rows",
             "an rnn_ac with a shared GRU / biGRU reader, (256, 256) ReLU heads and contiguous float32 parameters on a GPU"),
    "rnn_tiles": ("bf16", "rvo3d_policy_mlp_sample", "rvo3d_policy_rnn_tiles", _RNN_NEEDS),
    "rnn_tiles_x3": ("x3", "rvo3d_policy_mlp_x3_sample", "rvo3d_policy_rnn_tiles_x3", _RNN_NEEDS),
}


def _p(t):
    return C.c_void_p(t.data_ptr())


def check_state_dim(ac, env):
    """An rnn_ac reads the first state_dim floats of a row as the state and the rest as rows of 9; the env says how many
    state floats its rows hold (BuildingObsEnv.state_dim = 12 + 6k, 12 + 8k with building_velocity; 12 without the
    attribute).  A reader made for another number would take building floats for velocity obstacles - silently, where the
    difference is a multiple of 9."""
    reader = getattr(getattr(ac, "pi", None), "rnn_reader", None)
    have, want = getattr(reader, "state_dim", None), int(getattr(env, "state_dim", 12))
    if have is not None and int(have) != want:
        raise ValueError(f"the policy's reader was built with state_dim={int(have)}, the env's observation rows hold "
                         f"state_dim={want} state floats: build rnn_ac(..., state_dim={want})")


class KernelPolicyStep:
    """The policy step of `ac` on `rows` observation rows of width `obs_width` as the launches of `kind`.  Owns the
    scratch the launches share - features [rows, width], the list of rows with VO rows [rows], [count, finished
    workgroups], the tiles kernels' work area - at fixed addresses for its life (captured launches hold them).
    `option`: how the caller's user asked for this kind; a model that does not fit raises ValueError(f"{option} needs ...")."""

    KINDS = tuple(_KINDS)

    @staticmethod
    def plans(ac, kind, obs_width, option=None):
        """(the packed MLP / the zero-VO plan, the tiles blob or None) of a model that fits `kind`.  One that does not:
        None - or, asked for by `option`, ValueError(f"{option} needs ...")."""
        if kind not in _KINDS:
            raise ValueError(f"kind must be one of {', '.join(map(repr, _KINDS))}, not {kind!r}")
        precision, found = _KINDS[kind][0], None
        if kind in ("mlp", "mlp_x3"):
            mb = ac.mlp_blob(precision) if hasattr(ac, "mlp_blob") else None
            if mb is not None and ac.obs_width == obs_width:
                found = (mb, None)
        else:
            zp = ac.zero_vo_plan(precision) if hasattr(ac, "zero_vo_plan") else None
            if zp is not None and kind == "rnn0":
                found = (zp, None) if zp["rows_net"] is not None else None
            elif zp is not None:
                tb, vo = ac.rnn_tiles_blob(precision), obs_width - zp["state_dim"]
                found = (zp, tb) if tb is not None and vo % 9 == 0 and 1 <= vo // 9 <= 12 else None
        if found is None and option is not None:
            raise ValueError(f"{option} needs {_KINDS[kind][3]}")
        return found

    @classmethod
    def fits(cls, ac, kind, obs_width):
        """Whether `ac` can run as `kind` on observations of this width (cheap: the models cache what they pack)."""
        return cls.plans(ac, kind, obs_width) is not None

    def __init__(self, ac, kind, obs_width, rows, option="this policy step", state_dim=12):
        """state_dim: the state floats in front of a row's velocity-obstacle rows (12; BuildingObsEnv.state_dim): where
        the MLP kernels' zero column groups start."""
        self.ac, self.kind, self.obs_width, self.rows, self.option = ac, kind, int(obs_width), int(rows), option
        self.state_dim = int(state_dim)
        plan, tiles = self.plans(ac, kind, self.obs_width, option)
        self.device = plan["blob"].device
        if kind not in ("mlp", "mlp_x3"):
            self.slots = (self.obs_width - plan["state_dim"]) // 9
            i32 = dict(dtype=torch.int32, device=self.device)
            self._feat = torch.empty((self.rows, plan["width"]), dtype=torch.float32, device=self.device)
            self._list = torch.zeros(self.rows, **i32)
            self._count = torch.zeros(2, **i32)   # [count, finished workgroups]: the kernels leave both at zero
            if tiles is not None:
                nbytes = int(_lib.lib().rvo3d_policy_rnn_tiles_work_bytes(self.rows, self.slots))
                self._work = torch.zeros(nbytes // 4, **i32)
        self.refresh()

    def refresh(self):
        """Fetch the model's current plans (cached there; repacked in place when a parameter changed)."""
        self._plan, self._tiles = self.plans(self.ac, self.kind, self.obs_width, self.option)
        self.blob_ptr = self._plan["blob"].data_ptr()   # (what a captured launch holds; fixed: repacked in place)
        if self.kind == "rnn0":
            self._plan["rows_net"].slots = self.slots   # (a repacked plan has a new rows_net)

    def clear(self):
        """Zero the list's two counters and the work area's cursors.  The kernels leave them at zero; a rollout that was
        interrupted half-way may not have."""
        if self.kind not in ("mlp", "mlp_x3"):
            self._count.zero_()
        if self._tiles is not None:
            self._work[:32].zero_()

    def launch(self, obs, cnt, act, logp, val, std_factor, seed, step):
        """The step's launches on torch's current stream of the model's device: obs [rows, obs_width] float32 (row stride
        obs.stride(0)), cnt [rows] int32 -> act [rows, 3], logp [rows], val [rows] float32.  Noise from (seed, step).  No
        allocation, no host read, no synchronisation."""
        L, rows, plan, tb = _lib.lib(), self.rows, self._plan, self._tiles
        _, mlp, listed, _ = _KINDS[self.kind]
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        tanh = 1 if plan["tanh"] else 0
        sample = (_p(self.ac.log_std), std_factor, seed, step, _p(act), _p(logp), _p(val))
        # the MLP kernel's input: the observation with the env's counts (column groups of 9 behind the first 12 that are
        # zero for all rows of a wave are skipped; state_dim in place of 12 for wider rows), or the collapsed layer's features
        x, width, groups = obs, self.obs_width, (_p(cnt), self.state_dim, 9)
        if listed is not None:
            x, width, groups = self._feat, plan["width"], (None, 0, 0)
            lst, count, done_blocks = _p(self._list), _p(self._count), C.c_void_p(self._count.data_ptr() + 4)
            _lib.check(L.rvo3d_reader_zero_features(_p(obs), obs.stride(0), rows, plan["state_dim"], plan["feat_dim"],
                                                    _p(plan["ln_w"]), _p(plan["ln_b"]), plan["sum_h0"], plan["sumsq_h0"],
                                                    plan["eps"], _p(x), x.stride(0), _p(cnt), lst, count, st),
                       "rvo3d_reader_zero_features")
        _lib.check(getattr(L, mlp)(_p(plan["blob"]), width, _p(x), x.stride(0), rows, *groups, tanh, *sample, None, None, st),
                   mlp)
        if tb is not None:
            _lib.check(getattr(L, listed)(
                _p(tb["blob"]), tb["blob_bytes"], tb["hidden"], tb["in_dim"], tb["state_dim"], tb["bidir"], _p(obs),
                obs.stride(0), _p(cnt), lst, count, done_blocks, _p(self._work), rows, self.slots,
                1 if tb["tanh"] else 0, *sample, None, st), listed)
        elif listed is not None:
            _lib.check(L.rvo3d_policy_rows(C.byref(plan["rows_net"]), _p(obs), obs.stride(0), _p(cnt), lst, count,
                                           done_blocks, tanh, *sample, st), listed)
