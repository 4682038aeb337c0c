"""Evaluation rollouts: counterpart of `train/policy/post_train.py` (post_train.policy_test,
:38-128), batched over the E envs of a `BatchedDroneEnv` and reduced on the device.

Reference semantics kept:
  * action = acceler_vel * np.round(model.act(o, std_factor), 2) + drone.vel   (:63-74; the
    float32 product is widened and added to the float64 velocity, and - unlike the trainer's
    glue, multi_ppo.py:205 - NOT rounded again), through the plain `drone_step`;
  * per step the mean of ||vel|| over the drones of the env AFTER the step (:78-80);
  * an episode ends when any drone collided, at `max_ep_len`, or when every drone finished
    (:86: np.max(d) or ep_len == max_ep_len or np.min(finish)); the whole env is reset (:100);
  * an episode with every arrive flag set contributes its length (:89-90: np.min(info));
    it is a success when every drone finished (:104-105);
  * results: success rate over `num_episodes`, mean / std episode length of the "arrived"
    episodes and mean / std of the per-episode mean speed, np.round(., 2) (:116-128), one line
    appended to result_path + result_name.
With E envs in parallel every env contributes the same number of episodes: its first
ceil(num_episodes / E) ones (counting "the first num_episodes episodes to end" over all envs
would favour short episodes - collisions - and bias every statistic).  The statistics are over
those E * ceil(num_episodes / E) episodes; E = 1 is the reference's sequential loop exactly
(pinned by tests/golden/post_train_*.npz, produced by the reference's policy_test itself).
A "math domain error" (env_train=False: the reference's evaluator aborts when two drones
approach inside r + mr, vel_obs3D.py:13) is raised at the end of the step it happens in.

fused=True (opt-in) keeps the whole step on the device and the host out of the episode: policy ->
rvo3d_eval_action (the glue above, one kernel) -> the plain env step -> rvo3d_eval_account (the
bookkeeping above for every env, finished episodes recorded on the device) -> reset of the envs
that ended -> rvo3d_observe_envs (ONLY those envs are re-observed).  The host reads one counter
(and, with env_train=False, the error word) every `poll_every` steps; an error is raised at that
poll - also one of the at most poll_every - 1 uncounted steps behind the last record.  The
records are sorted by (step, env) - the order in which the loop above appends - and go through
`summarize_records`.  Per env this is the reference's loop exactly: an env in mid-episode keeps
the observation of its step (ir_gym.observation_reward, with the action).  The unfused loop
re-observes EVERY env with action = 0 (ir_gym.env_observation) whenever any env ended, so with
E > 1 and a policy that looks at its observation an env's trajectory there depends on its
neighbours' episode ends; with E = 1 the two loops agree.

safety=True (opt-in, either loop) adds the safety figures of the field to the result: per episode the minimum separation
between two drones, the minimum clearance to a building and to a map face, and the near-miss pair-steps (pairs within
near_margin of touching), from rvo3d_safety_scan on the state behind every step (the rules: include/rvo3d.h).  The fused
loop calls rvo3d_eval_account_safety in place of rvo3d_eval_account, which folds them into four more record arrays on
the device; the host loop calls env.safety() and folds by the same rules.  `policy_test` returns what it returns
without it and leaves the summary (rvo3d_amd.safety.summarize_safety) in self.safety.

shield=dict(...) (opt-in, either loop, every policy_type) puts the action shield behind the controller: the action that
would go to env.step - eval_action's output for "drl", _action()'s otherwise - goes through env.shield_action(**shield)
first (rvo3d_shield_action, include/rvo3d.h: the action comes back untouched where the velocity it would fly satisfies
the ORCA planes of the current state, and as the command for the nearest permitted velocity where it does not).  One more
launch per step and no host synchronisation: the evaluator owns one [E, 4] int64 tensor of totals on the device for the
whole policy_test, which every call adds to, and reads it once at the end into self.shield: `judged` (drone-steps the
shield judged) and `intervened_share`, `fallback_share` (no permitted velocity: ORCA's fallback) and `clipped_share`
(intervened with a command that clipped), each over `judged`.  The totals are over ALL steps flown: the episodes beyond
an env's quota, which the records do not count, and with fused=True the at most poll_every - 1 steps behind the last
record are included.  Shielding inside the trainer's rollouts is out of scope: the stored action, its log-probability
and the flown action would diverge.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib
from ..safety import summarize_safety
from .policy_step import KernelPolicyStep, check_state_dim

# bits of a record's flag byte (rvo3d_eval_account)
REC_ARRIVED, REC_FINISHED, REC_COLLIDED, REC_TIMEOUT = 1, 2, 4, 8


def summarize_records(step, env, length, ret, speed, flags, policy_name="policy"):
    """The evaluation's result from its episode records (plain numpy arrays, one entry per counted
    episode, any order): sorted by (step, env) - the order in which the sequential loop meets them -
    they give the returned dict, the result line and the per-episode lines of `inf_print`
    (post_train.py:89-128).  Returns (result, line, episode_lines)."""
    step, env = np.asarray(step), np.asarray(env)
    order = np.lexsort((env, step))
    length = np.asarray(length)[order]
    ret = np.asarray(ret, dtype=np.float64)[order]
    speed = np.asarray(speed, dtype=np.float64)[order]
    flags = np.asarray(flags)[order].astype(np.int64)
    arrived = (flags & REC_ARRIVED) != 0
    total = len(order)
    sn = int(((flags & REC_FINISHED) != 0).sum())
    ep_len_list = [int(x) for x in length[arrived]]
    mean_speed_list = [float(x) for x in speed]
    ep_ret_list = [float(x) for x in ret]
    episode_lines = ["%s, Episode %d \t EpRet %.3f \t EpLen %d \t EpSpeed  %.3f"
                     % ("Successful" if arrived[n] else "Fail", n, ret[n], length[n], speed[n]) for n in range(total)]
    mean_len = 0 if not ep_len_list else np.round(np.mean(ep_len_list), 2)
    std_len = 0 if not ep_len_list else np.round(np.std(ep_len_list), 2)
    average_speed = np.round(np.mean(mean_speed_list), 2)
    std_speed = np.round(np.std(mean_speed_list), 2)
    line = ("policy_name: " + policy_name + "  successful rate: {:.2%}".format(sn / total)
            + " average EpLen: %s std length %s average speed: %s std speed %s"
            % (mean_len, std_len, average_speed, std_speed))
    result = dict(success_rate=sn / total, mean_len=float(mean_len), std_len=float(std_len),
                  average_speed=float(average_speed), std_speed=float(std_speed),
                  episodes=total, ep_ret=ep_ret_list, ep_len=ep_len_list, speed=mean_speed_list)
    return result, line, episode_lines


class post_train:
    def __init__(self, env, num_episodes=100, max_ep_len=150, acceler_vel=1.0, render=False,
                 save=False, neighbor_region=4, neighbor_num=5, args=None, fused=False, policy_kernel=None,
                 poll_every=8, seed=0, safety=False, near_margin=0.5, rvo=None, command="raw", shield=None, **kwargs):
        """fused: the device-side loop (module docstring); policy_kernel: None (policy.step_tensors) or the
        KernelPolicyStep kind that runs the policy - "mlp", "mlp_x3" (the MLP actor-critic, bf16 / float32-class),
        "rnn_tiles" or "rnn_tiles_x3" (the biGRU actor-critic, likewise) - either loop; poll_every: steps between two host
        reads of the fused loop; seed: of the kernels' counter-based noise; safety / near_margin: the safety figures (module
        docstring), off by default: neither loop then makes a launch it did not make before; rvo: keyword arguments of the
        classical controller policy_test flies for policy_type "rvo" (env.rvo_vel), "rvo_city" (env.rvo_vel_city) and
        "orca" (env.orca_vel); command: what becomes of the controller's velocity (policy types without a network) - "raw":
        handed to env.step as it is, which reads it as acceleration, yaw and pitch increments (the reference's glue);
        "velocity": through env.velocity_command first, so that the step flies that velocity; shield: None, or the keyword
        arguments of env.shield_action that every action goes through before the step (module docstring)."""
        if command not in ("raw", "velocity"):
            raise ValueError(f"command must be 'raw' or 'velocity', not {command!r}")
        self.command = command
        if policy_kernel not in (None, "mlp", "mlp_x3", "rnn_tiles", "rnn_tiles_x3"):
            raise ValueError("policy_kernel must be None, 'mlp', 'mlp_x3', 'rnn_tiles' or 'rnn_tiles_x3', "
                             f"not {policy_kernel!r}")
        if int(poll_every) < 1:
            raise ValueError("poll_every must be >= 1")
        self.fused, self.policy_kernel, self.poll_every, self.seed = bool(fused), policy_kernel, int(poll_every), int(seed)
        self.with_safety, self.near_margin = bool(safety), float(near_margin)
        if not (np.isfinite(self.near_margin) and self.near_margin >= 0.0):
            raise ValueError("near_margin must be finite and >= 0")
        self.safety = None   # summarize_safety's dict once policy_test ran with safety=True
        self.rvo = dict(rvo or {})
        if "diagnostics" in self.rvo:
            raise ValueError("rvo= carries the controller's parameters, not diagnostics")
        self.shield_args = None if shield is None else dict(shield)
        if self.shield_args is not None and {"diagnostics", "totals"} & set(self.shield_args):
            raise ValueError("shield= carries the shield's parameters, not diagnostics or totals")
        self.shield = None   # the shield's shares once policy_test ran with shield=dict(...)
        self.env = env
        self.num_episodes = num_episodes
        self.max_ep_len = max_ep_len
        self.acceler_vel = acceler_vel
        self.render, self.save = render, save  # accepted for signature parity; plotting is out of scope
        self.drone_number = env.N
        self.inf_print = kwargs.get("inf_print", True)
        self.std_factor = kwargs.get("std_factor", 0.001)
        self.nr, self.nm = neighbor_region, neighbor_num
        self.args = args

    # -- policy ---------------------------------------------------------------------------
    def load_policy(self, policy, std_factor=1, policy_dict=False):
        """`policy`: an actor-critic module (rnn_ac / mlp_ac), or the path of a checkpoint
        written by multi_ppo.save_model (state dict under 'model_state', loaded with
        weights_only=True into `self.args.ac`; the reference's full-module pickles
        (post_train.py:143) are not loaded)."""
        if isinstance(policy, (str, bytes)) or hasattr(policy, "__fspath__"):
            ac = getattr(self.args, "ac", None)
            if ac is None:
                raise ValueError("loading a checkpoint needs args.ac (the module to load into)")
            ck = torch.load(policy, map_location=self.env.device, weights_only=True)
            ac.load_state_dict(ck["model_state"], strict=True)
            policy = ac
        policy.eval()
        check_state_dim(policy, self.env)
        if self.policy_kernel is not None:
            return self._kernel_policy(policy, std_factor)

        def get_action(obs, cnt):  # batched model.act(x, std_factor), stays on the device
            a, _, _ = policy.step_tensors((obs, cnt), std_factor)
            return a.float()

        return get_action

    def _kernel_policy(self, policy, std_factor):
        """model.act as the launches of KernelPolicyStep(self.policy_kernel) - the trainer's, with the evaluator's
        std_factor; noise from (seed, number of calls so far)."""
        env = self.env
        rows = env.E * env.N
        step = KernelPolicyStep(policy, self.policy_kernel, env.W, rows, option=f"policy_kernel={self.policy_kernel!r}",
                                state_dim=getattr(env, "state_dim", 12))
        f32 = dict(dtype=torch.float32, device=env.device)
        act, logp, val = torch.empty((rows, 3), **f32), torch.empty(rows, **f32), torch.empty(rows, **f32)  # logp, val: scratch
        calls = [0]

        def get_action(obs, cnt):
            step.refresh()   # (cached; repacked when a parameter changed)
            step.launch(obs, cnt, act, logp, val, float(std_factor), self.seed, calls[0])
            calls[0] += 1
            return act

        return get_action

    # -- evaluation -------------------------------------------------------------------------
    def _classical(self, policy_type):
        """What both loops fly without a network: "rvo" - env.rvo_vel, "rvo_city" - env.rvo_vel_city, "orca" -
        env.orca_vel, each with the constructor's rvo= parameters; any other policy_type - env.des_vel."""
        env = self.env
        if policy_type == "rvo":
            return lambda: env.rvo_vel(**self.rvo)
        if policy_type == "rvo_city":
            return lambda: env.rvo_vel_city(**self.rvo)
        if policy_type == "orca":
            return lambda: env.orca_vel(**self.rvo)
        return env.des_vel

    def _action(self):
        """The action of a step without a network: _fly()'s velocity, by the constructor's command=."""
        v = self._fly()
        return self.env.velocity_command(v) if self.command == "velocity" else v

    def _shielded(self, action):
        """The action env.step gets: through env.shield_action with shield=dict(...), else as it is."""
        if self.shield_args is None:
            return action
        return self.env.shield_action(action, totals=self._shield_totals, **self.shield_args)

    def _shield_summary(self):
        """self.shield from the totals on the device: the one host read of the shield (module docstring)."""
        if self.shield_args is None:
            return
        judged, intervened, fallback, clipped = (int(x) for x in self._shield_totals.sum(dim=0).cpu())
        share = lambda n: n / judged if judged else 0.0
        self.shield = dict(judged=judged, intervened_share=share(intervened), fallback_share=share(fallback),
                           clipped_share=share(clipped))

    def policy_test(self, policy_type="drl", policy_path=None, policy_name="policy", result_path=None,
                    result_name="/result.txt", policy=None, policy_dict=False, **_unused):
        env = self.env
        E, N, dev = env.E, env.N, env.device
        act_fn = None
        self._fly = self._classical(policy_type)
        if self.shield_args is not None:
            self._shield_totals = torch.zeros((E, 4), dtype=torch.int64, device=dev)
        if policy_type == "drl":
            act_fn = self.load_policy(policy if policy is not None else policy_path,
                                      self.std_factor, policy_dict=policy_dict)
        if self.fused:
            return self._policy_test_fused(act_fn, policy_name, result_path, result_name)
        env.reset()
        obs, cnt = env.observe()
        ep_len = torch.zeros(E, dtype=torch.int64, device=dev)
        ep_ret = torch.zeros(E, dtype=torch.float64, device=dev)
        speed_sum = torch.zeros(E, dtype=torch.float64, device=dev)
        n = 0
        records = []   # (length, return, speed, flags) of every counted episode, in the order the loop meets them
        quota = -(-self.num_episodes // E)   # episodes counted per env
        counted = [0] * E
        total = quota * E
        check_domain = not getattr(env, "env_train", True)
        # drone counts (BatchedDroneEnv.set_drone_counts): the reductions over an env's drones range over the drones it
        # has, as rvo3d_eval_account makes them on the fused path; `ghost` is None without counts
        counts = getattr(env, "drone_counts", None)
        ghost = None if counts is None else ~env.live
        if self.with_safety:   # running minima / near pair-steps of every env's episode, folded as rvo3d_eval_account_safety folds
            inf = torch.full((E,), float("inf"), dtype=torch.float64, device=dev)
            run = [inf.clone(), inf.clone(), inf.clone(), torch.zeros(E, dtype=torch.int64, device=dev)]
            safety_records = []   # (min_sep, min_bclear, min_wall, near, drones) per counted episode
            drones_of = np.full(E, N) if counts is None else counts.cpu().numpy()
        while n < total:
            if act_fn is not None:
                a = act_fn(obs.view(-1, env.W), cnt.view(-1)).view(E, N, 3)
                # np.round(float32, 2) = rint(a * 100) / 100 with a TRUE division (a tensor
                # divisor: torch turns a scalar divisor into a multiplication by 1/100)
                a_inc = torch.round(a * 100.0) / torch.full_like(a, 100.0)
                vel = env.vel                                              # [E, N, 3] float64
                action = (torch.as_tensor(self.acceler_vel, dtype=torch.float32, device=dev) * a_inc).double() + vel
            else:
                action = self._action()
            action = self._shielded(action)
            obs, cnt, rew, done, info, fin = env.step(action)             # plain drone_step
            if ghost is None:
                speed_sum += torch.linalg.vector_norm(env.vel, dim=-1).mean(dim=1)
                all_fin, all_info = fin.bool().all(dim=1), info.bool().all(dim=1)
            else:
                speed_sum += torch.linalg.vector_norm(env.vel, dim=-1).masked_fill(ghost, 0.0).sum(dim=1) / counts.double()
                all_fin, all_info = (fin.bool() | ghost).all(dim=1), (info.bool() | ghost).all(dim=1)
            ep_ret += rew[:, 0].double()                                   # r[0] (post_train.py:82)
            ep_len += 1
            ended = done.bool().any(dim=1) | (ep_len == self.max_ep_len) | all_fin   # (a ghost's done byte is 0)
            if self.with_safety:   # the state behind the step, before any reset; ghost rows are +inf
                s_sep, s_bclear, s_wall, s_near = env.safety(self.near_margin)
                for k, v in enumerate((s_sep, s_bclear, s_wall)):
                    m = v.min(dim=1).values
                    run[k] = torch.where(m < run[k], m, run[k])
                run[3] = run[3] + s_near.to(torch.int64)
            if check_domain:
                # ONE read of the (read-and-clear) error word per step; both bits are acted on here, so
                # nothing is lost to the clear.  With E > 1 the word is not attributed to an env: the
                # whole evaluation aborts, where the reference's sequential loop (E = 1) loses the one
                # episode it was in - evaluate with E = 1 for the reference's exact abort semantics.
                flags = env.error_flags()
                if flags & 2:
                    raise ValueError("math domain error")  # the reference's drone_step raised here
                if flags & 1:
                    raise ValueError("observation contains NaN/Inf")  # ir_gym.py:232-239
            if bool(ended.any()):
                arrived, success = all_info, all_fin
                idx = torch.nonzero(ended).flatten().tolist()
                el, sp, er = ep_len.cpu().numpy(), (speed_sum / ep_len.double()).cpu().numpy(), ep_ret.cpu().numpy()
                ar, su = arrived.cpu().numpy(), success.cpu().numpy()
                if self.with_safety:
                    rs = [r.cpu().numpy() for r in run]
                for e in idx:
                    if counted[e] >= quota:
                        continue  # this env has delivered its share; it keeps stepping, uncounted
                    counted[e] += 1
                    if self.inf_print:
                        print("%s, Episode %d \t EpRet %.3f \t EpLen %d \t EpSpeed  %.3f"
                              % ("Successful" if ar[e] else "Fail", n, er[e], el[e], sp[e]))
                    records.append((el[e], er[e], sp[e], (REC_ARRIVED if ar[e] else 0) | (REC_FINISHED if su[e] else 0)))
                    if self.with_safety:
                        safety_records.append((rs[0][e], rs[1][e], rs[2][e], rs[3][e], drones_of[e]))
                    n += 1
                env.reset(ended)
                obs, cnt = env.observe()
                z = torch.zeros_like(ep_len)
                ep_len = torch.where(ended, z, ep_len)
                ep_ret = torch.where(ended, torch.zeros_like(ep_ret), ep_ret)
                speed_sum = torch.where(ended, torch.zeros_like(speed_sum), speed_sum)
                if self.with_safety:
                    run = [torch.where(ended, inf, r) for r in run[:3]] + [torch.where(ended, torch.zeros_like(run[3]), run[3])]
        self._shield_summary()
        length, ret, speed, flags = zip(*records)
        if self.with_safety:
            ms, mb, mw, nr, dr = (np.asarray(x) for x in zip(*safety_records))
            self.safety_records = dict(rec_min_sep=ms, rec_min_bclear=mb, rec_min_wall=mw, rec_near=nr)
            self.safety = summarize_safety(ms, mb, mw, nr, length, dr)
        result, line, _ = summarize_records(np.arange(n), np.zeros(n, dtype=np.int64), length, ret, speed, flags, policy_name)
        if result_path is not None:
            with open(result_path + result_name, "a") as f:
                print(line, file=f)
        if self.inf_print:
            print(line)
        return result

    def _policy_test_fused(self, act_fn, policy_name, result_path, result_name):
        """The same evaluation with the episodes accounted for on the device (module docstring)."""
        env = self.env
        E, N, dev = env.E, env.N, env.device
        quota = -(-self.num_episodes // E)   # episodes counted per env
        total = quota * E
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        t = dict(ep_len=z(E, torch.int32), ep_ret=z(E, torch.float64), speed_sum=z(E, torch.float64),
                 counted=z(E, torch.int32), rec_len=z((E, quota), torch.int32), rec_ret=z((E, quota), torch.float64),
                 rec_speed=z((E, quota), torch.float64), rec_step=z((E, quota), torch.int64),
                 rec_flags=z((E, quota), torch.uint8), remaining=torch.full((1,), total, dtype=torch.int32, device=dev),
                 ended=z(E, torch.uint8))
        bufs = _lib.EvalBufs(**{k: v.data_ptr() for k, v in t.items()})
        rec_keys = ("rec_step", "rec_len", "rec_ret", "rec_speed", "rec_flags")
        if self.with_safety:
            inf = lambda shape: torch.full(shape, float("inf"), dtype=torch.float64, device=dev)
            ts = dict(ep_min_sep=inf((E,)), ep_min_bclear=inf((E,)), ep_min_wall=inf((E,)), ep_near=z(E, torch.int64),
                      rec_min_sep=inf((E, quota)), rec_min_bclear=inf((E, quota)), rec_min_wall=inf((E, quota)),
                      rec_near=z((E, quota), torch.int64))
            sbufs = _lib.EvalSafetyBufs(**{k: v.data_ptr() for k, v in ts.items()})
            t.update({k: v for k, v in ts.items() if k.startswith("rec_")})
            rec_keys += ("rec_min_sep", "rec_min_bclear", "rec_min_wall", "rec_near")
        L = _lib.lib()
        p = lambda x: C.c_void_p(x.data_ptr())
        check_domain = not getattr(env, "env_train", True)
        env.reset()
        obs, cnt = env.observe()
        step = 0
        while True:
            if act_fn is not None:
                a = act_fn(obs.view(-1, env.W), cnt.view(-1)).view(E, N, 3)
                action = env.eval_action(a, self.acceler_vel)
            else:
                action = self._action()
            action = self._shielded(action)
            obs, cnt, rew, done, info, fin = env.step(action)             # plain drone_step
            if self.with_safety:
                _lib.check(L.rvo3d_eval_account_safety(env._h, p(rew), p(done), p(info), p(fin), self.max_ep_len, quota,
                                                       step, C.byref(bufs), self.near_margin, C.byref(sbufs),
                                                       env._stream()), "rvo3d_eval_account_safety")
            else:
                _lib.check(L.rvo3d_eval_account(env._h, p(rew), p(done), p(info), p(fin), self.max_ep_len, quota, step,
                                                C.byref(bufs), env._stream()), "rvo3d_eval_account")
            env.reset(t["ended"])
            obs, cnt = env.observe_envs(t["ended"])
            step += 1
            if step % self.poll_every == 0:
                if check_domain:
                    flags = env.error_flags()   # (read-and-clear; both bits are acted on here)
                    if flags & 2:
                        raise ValueError("math domain error")
                    if flags & 1:
                        raise ValueError("observation contains NaN/Inf")
                if int(t["remaining"].item()) <= 0:
                    break
        self._shield_summary()
        e_idx = np.repeat(np.arange(E), quota)   # env of record [e][k]; remaining <= 0: every slot is filled
        # the records as the device left them, [E][quota] each (kept for the caller: self.records)
        rec = self.records = {k: t[k].cpu().numpy() for k in rec_keys}
        if self.with_safety:
            counts = getattr(env, "drone_counts", None)
            drones = np.repeat(np.full(E, N) if counts is None else counts.cpu().numpy(), quota)
            self.safety = summarize_safety(rec["rec_min_sep"], rec["rec_min_bclear"], rec["rec_min_wall"], rec["rec_near"],
                                           rec["rec_len"].reshape(-1), drones)
        flat = {k: v.reshape(-1) for k, v in rec.items()}
        result, line, episode_lines = summarize_records(flat["rec_step"], e_idx, flat["rec_len"], flat["rec_ret"],
                                                        flat["rec_speed"], flat["rec_flags"], policy_name)
        if self.inf_print:
            for ln in episode_lines:
                print(ln)
        if result_path is not None:
            with open(result_path + result_name, "a") as f:
                print(line, file=f)
        if self.inf_print:
            print(line)
        return result
