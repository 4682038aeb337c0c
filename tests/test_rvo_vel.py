"""Classical RVO velocity selection (reciprocal_vel_obs.py).
CPU: the oracle (a) call by call against what the reference class's OWN methods return where they
run on an instance - preprocess, penalty, distance, the candidate grid of vel_candidate, the
inside branch of vel_select (tests/golden/rvo_calls.npz) - and (b) as a whole against vectors made
with the reference's helper functions (rvo_vel.npz; oracle/gen_golden_rvo.py makes both).
GPU: the HIP kernel against the oracle, with the knife-edge accounting of the step tests - on random
scenes, and on a table of scenes built to reach the paths those almost never take (every live candidate
inside a velocity obstacle, no live candidate, per-drone radius and priority, five and eight waves, the
ends of the accepted arguments; the oracle reports which path each agent took, a CPU test holds the table
to it).
cal_vel itself, config_vo and vo_out2 raise in the reference: the loop around the pinned parts is
"parity unpinned" (DESIGN.md section 7)."""
import collections
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "3drvo-marl-collisionavoidance_amd")]
import oracle as orc  # noqa: E402


def cases():
    z = np.load(os.path.join(HERE, "golden", "rvo_vel.npz"))
    for k in range(int(z["n_cases"])):
        yield {n[len(f"c{k}_"):]: z[n] for n in z.files if n.startswith(f"c{k}_")}


def test_oracle_matches_vectors_made_with_the_reference_helpers():
    n = 0
    for c in cases():
        env = orc.OracleEnv(c["waypoints"], c["n_points"], c["map_size"], None, nm=10)
        env.set_state(pos=c["pos"], vel=c["vel"])
        np.testing.assert_array_equal(env.des_vel(), c["des"])
        got = env.rvo_vel(tuple(c["vmax"]), float(c["acceler"]))
        np.testing.assert_array_equal(got, c["out"])
        n += got.shape[0] * got.shape[1]
    assert n == 168


def calls():
    return np.load(os.path.join(HERE, "golden", "rvo_calls.npz"))


def test_preprocess_matches_the_reference_method():
    """reciprocal_vel_obs.preprocess (:32-54): the 10 m neighbour gate (norm == 10 stays, the very
    same position stays too) and this class's own building gate (h > z - 1, <= 10 m in the plane)."""
    z = calls()
    kept = 0
    for a, d, b, kd, kb in zip(z["pre_agent"], z["pre_drones"], z["pre_blds"], z["pre_keep_d"], z["pre_keep_b"]):
        gd, gb = orc.rvo_preprocess(a, d, b)
        assert np.array_equal(gd, kd.astype(bool)) and np.array_equal(gb, kb.astype(bool))
        assert gd[3] and not gd[2]                          # the very same spot stays; 10 m + 5 um does not
        kept += int(gd.sum())
    # drones 0 / 1 sit 6-8-0 / 0-6-8 away from 2-decimal coordinates: |d| = 10 up to the rounding of the
    # sums, so the <= 10 gate falls either way - whatever the reference's own norm says is what counts
    assert 0 < int(z["pre_keep_d"][:, :2].sum()) < 120
    assert 100 < kept < 60 * 12 and 0 < int(z["pre_keep_b"].sum()) < 60 * 8


def test_penalty_distance_and_inside_selection_match_the_reference_methods():
    """reciprocal_vel_obs.penalty (:126-147: tc_min over the neighbours, inf for tc_min == 0, 0 for
    no collision course), .distance, and vel_select's inside branch (min by penalty, first of equals)."""
    z = calls()
    for k in range(len(z["pen_n"])):
        n, n_in = int(z["pen_n"][k]), int(z["pen_n_in"][k])
        ag, od = z["pen_agent"][k], z["pen_odro"][k][:n]
        got = orc.rvo_penalty(z["pen_vel"][k], z["pen_des"][k], ag[:8], od, 1.0)
        assert got == z["pen_pen"][k] or (np.isnan(got) and np.isnan(z["pen_pen"][k])), k
        assert orc.rvo_distance(z["pen_vel"][k], z["pen_des"][k]) == z["pen_dist"][k]
        assert orc.rvo_select_inside(z["pen_inside"][k][:n_in], ag, od) == int(z["pen_sel"][k]), k
    assert np.isinf(z["pen_pen"]).sum() > 5 and (z["pen_pen"] == z["pen_dist"]).sum() > 5  # both ends of 1/tc


def test_candidate_grid_matches_vel_candidate():
    """reciprocal_vel_obs.vel_candidate (:85-101) with an empty VO list returns the candidate grid
    itself: np.arange over the clipped range per axis, |v| >= 0.3, x outermost."""
    z = calls()
    sizes = set()
    for v, vm, acc, n, cand in zip(z["cand_vel"], z["cand_vmax"], z["cand_acc"], z["cand_n"], z["cand_cand"]):
        got = orc.rvo_candidates(v, vm, float(acc))
        assert len(got) == int(n)
        np.testing.assert_array_equal(got, cand[:int(n)])
        sizes.add(int(n))
    assert 0 in sizes and max(sizes) >= 27 and len(sizes) > 5


def test_what_does_not_run_in_the_reference_is_on_record():
    z = calls()
    assert str(z["raises_config_vo"]) == "ValueError"                    # :63-83, state[0:4] into get_PAA
    assert str(z["raises_vel_candidate_with_vo"]) == "AttributeError"    # :109, list.append assignment
    assert str(z["raises_cal_vel"]) != ""                                # the driver itself
    assert bool(z["vel_select_outside_returns_none"])                    # :119-124, missing return


@pytest.mark.gpu
def test_hip_rvo_vel_matches_oracle():
    import torch
    from rvo3d_amd import BatchedDroneEnv, synthetic_world
    from test_gpu_parity import Tally
    rng = np.random.default_rng(7)
    agents = 0
    for (E, N, L, acc, vmax) in [(64, 16, 8.0, 0.5, (2.0, 2.0, 2.0)), (16, 64, 12.0, 1.0, (2.0, 2.0, 2.0)),
                                 (8, 100, 14.0, 0.5, (1.0, 1.5, 1.0)), (32, 5, 4.0, 0.75, (2.0, 2.0, 1.0)),
                                 (4, 256, 30.0, 0.5, (2.0, 2.0, 2.0))]:
        w = synthetic_world(E, N, (L, L, L), seed=int(rng.integers(1 << 30)), min_sep=0.5)
        env = BatchedDroneEnv(w, neighbors_num=10)
        ref = orc.OracleEnv(w.waypoints, w.n_points, w.map_size, w.buildings, nm=10, threads=8)
        pos = np.round(w.waypoints[:, :, 0] + rng.uniform(-0.3, 0.3, (E, N, 3)), 2)
        vel = np.round(rng.uniform(-1.2, 1.2, (E, N, 3)), 2)
        vel[rng.random((E, N)) < 0.15] = 0.0
        env.set_state(pos=pos, vel=vel); ref.set_state(pos=pos, vel=vel)
        got = env.rvo_vel(vmax, acc).cpu().numpy()
        want = ref.rvo_vel(vmax, acc)
        # alpha = round(asin, 2) and beta = round(acos, 2) rest on libm results (glibc vs ocml: <= 1 ulp
        # apart): the oracle reports, per agent, how close any of its roundings came to a tie; only
        # agents within 1e-9 of one may differ, and they are counted (class Tally, as for the step)
        tl = Tally(f"rvo_vel/{N}x{E}", E)
        tl.begin(ref.margin())
        tl.check("rvo_vel", got == want)
        tl.end()
        tl.finish(agents=E * N)
        agents += E * N
        env.close()
    assert agents > 3000


# ---- the rare paths of vel_select, per-drone radius / priority, more than four waves, the argument edges ----------
# One table, replayed by a CPU test (does every scene still reach the paths it is here for?) and by a GPU test (does
# the kernel agree with the oracle on them?).  State recipe of test_hip_rvo_vel_matches_oracle: positions = first
# waypoint + U(-0.3, 0.3), velocities U(-vs, vs), both rounded to 2 decimals, 15 % of the velocities exactly 0.
# radius / priority: None = the reference's constants 0.2 / 5, a number = every drone, "per" = per drone (radius
# U(0.15, 0.6) rounded to 2 decimals, priority an integer 1..8).  floors: {code or flag: least number of agents}, far
# below what the oracle gives (DESIGN.md section 7 has the figures); only = the one code every agent must have.
OUT_ONLY, OUT_SOME_IN, IN_ONLY, NONE = orc.RVO_OUT_ONLY, orc.RVO_OUT_SOME_IN, orc.RVO_IN_ONLY, orc.RVO_NONE
OVERLAP, TC_ZERO, IN_FIRST, IN_NEAREST = "overlap", "tc_zero", "in_only_tc_zero", "in_only_tc_positive"
Scene = collections.namedtuple("Scene", "label E N L acceler vmax vs radius priority seed floors only",
                               defaults=(None, None, 0, {}, None))
V2 = (2.0, 2.0, 2.0)
VFLAT = (2.0, 1.5, 1.0)
SCENES = [
    Scene("dense_equal_radius", 16, 64, 6.0, 0.5, V2, 1.2, 0.4, None, 11,
          {IN_ONLY: 200, OUT_SOME_IN: 100, OVERLAP: 20, TC_ZERO: 20, IN_FIRST: 20, IN_NEAREST: 20}),
    Scene("dense_per_drone", 16, 64, 6.0, 0.5, V2, 1.2, "per", "per", 12,
          {IN_ONLY: 200, OUT_SOME_IN: 100, OVERLAP: 20, TC_ZERO: 20, IN_FIRST: 20, IN_NEAREST: 20}),
    Scene("slow", 8, 16, 8.0, 0.25, V2, 0.2, None, None, 13, {NONE: 3, IN_ONLY: 3, OUT_ONLY: 20}),
    Scene("five_waves", 2, 300, 10.0, 0.5, VFLAT, 1.2, "per", "per", 14, {IN_ONLY: 100, OUT_SOME_IN: 50}),
    Scene("eight_waves", 1, 512, 12.0, 1.0, VFLAT, 1.2, "per", "per", 15, {IN_ONLY: 100, OUT_SOME_IN: 50}),
    Scene("ring_seam_65", 3, 65, 6.0, 1.0, V2, 1.2, "per", "per", 16, {IN_ONLY: 40}),
    Scene("ring_seam_63", 5, 63, 6.0, 0.75, V2, 1.2, "per", "per", 17, {IN_ONLY: 60}),
    Scene("acceler_0", 8, 16, 8.0, 0.0, V2, 1.2, None, None, 18, {}, NONE),
    Scene("acceler_1", 8, 16, 12.0, 1.0, V2, 1.2, None, None, 19, {OUT_ONLY: 20, OUT_SOME_IN: 20}),
    # a zero component of vmax clips that axis to [0, 0]: np.arange(0, 0, 0.5) is empty, for every drone
    Scene("vmax_zero_component", 8, 16, 8.0, 0.5, (2.0, 0.0, 2.0), 1.2, None, None, 20, {}, NONE),
    # vmax below |v| - acceler on some axis of most drones: both ends of the clip land on vmax, no candidate; the
    # drones that are slow on all three axes keep theirs
    Scene("vmax_small", 8, 16, 5.0, 0.5, (0.2, 0.2, 0.2), 1.2, 0.5, None, 21, {NONE: 3, IN_ONLY: 3, OUT_ONLY: 3}),
]
SCENE_IDS = [s.label for s in SCENES]


def _per_drone(sc, rng, what):
    spec = getattr(sc, what)
    if spec != "per":
        return spec
    if what == "radius":
        return np.round(rng.uniform(0.15, 0.6, (sc.E, sc.N)), 2)
    return rng.integers(1, 9, (sc.E, sc.N)).astype(np.float64)


@functools.lru_cache(maxsize=None)
def scene_state(sc_index, equal_priority=False):
    """(world, pos, vel, radius, priority) of a scene; equal_priority: the same scene with the reference's constant."""
    from rvo3d_amd import synthetic_world
    sc = SCENES[sc_index]
    rng = np.random.default_rng(sc.seed)
    w = synthetic_world(sc.E, sc.N, (sc.L, sc.L, sc.L), seed=int(rng.integers(1 << 30)), min_sep=0.5)
    pos = np.round(w.waypoints[:, :, 0] + rng.uniform(-0.3, 0.3, (sc.E, sc.N, 3)), 2)
    vel = np.round(rng.uniform(-sc.vs, sc.vs, (sc.E, sc.N, 3)), 2)
    vel[rng.random((sc.E, sc.N)) < 0.15] = 0.0
    radius, priority = _per_drone(sc, rng, "radius"), _per_drone(sc, rng, "priority")
    return w, pos, vel, radius, None if equal_priority else priority


class OracleRun:
    """One scene through the oracle, computed once and shared by the tests (read-only)."""

    def __init__(self, w, pos, vel, radius, priority, vmax, acceler):
        E, N = pos.shape[:2]
        bc = lambda a: None if a is None else np.broadcast_to(np.asarray(a, np.float64), (E, N))
        self.ref = orc.OracleEnv(w.waypoints, w.n_points, w.map_size, w.buildings, nm=10, radius=bc(radius),
                                 priority=bc(priority), threads=8)
        self.ref.set_state(pos=pos, vel=vel)
        self.des = self.ref.des_vel()
        self.want = self.ref.rvo_vel(vmax, acceler)
        self.margin = self.ref.margin()
        self.branch, self.flags = self.ref.rvo_branch(), self.ref.rvo_flags()
        self.cs_near_one = self.ref.rvo_cs_near_one()
        for a in (self.des, self.want, self.margin, self.branch, self.flags, self.cs_near_one):
            a.setflags(write=False)

    def counts(self):
        c = {k: int((self.branch == k).sum()) for k in (OUT_ONLY, OUT_SOME_IN, IN_ONLY, NONE)}
        c[OVERLAP] = int((self.flags & orc.RVO_OVERLAP != 0).sum())
        c[TC_ZERO] = int((self.flags & orc.RVO_TC_ZERO != 0).sum())
        # inside-only agents by what decides among their candidates: the first one (penalty inf) / the distance
        c[IN_FIRST] = int(((self.branch == IN_ONLY) & (self.flags & orc.RVO_TC_ZERO != 0)).sum())
        c[IN_NEAREST] = c[IN_ONLY] - c[IN_FIRST]
        return c

    def tally_extra(self):
        c = self.counts()
        return dict(agents=self.branch.size, out_only=c[OUT_ONLY], out_some_in=c[OUT_SOME_IN], in_only=c[IN_ONLY],
                    none=c[NONE], overlap=c[OVERLAP], tc_zero=c[TC_ZERO], in_only_tc_zero=c[IN_FIRST])


@functools.lru_cache(maxsize=None)
def scene_oracle(sc_index, equal_priority=False):
    sc = SCENES[sc_index]
    return OracleRun(*scene_state(sc_index, equal_priority), sc.vmax, sc.acceler)


def knife_bound(samples):
    """Tally.finish's bound on the agents within 1e-9 of a rounding tie (test_gpu_parity.py)."""
    lim = 0.01 * samples
    return lim + 3.0 * np.sqrt(lim) + 2


@pytest.mark.parametrize("k", range(len(SCENES)), ids=SCENE_IDS)
def test_scene_reaches_the_paths_it_is_here_for(k):
    """The oracle alone: every scene of the table still sends at least `floors` agents down the paths of vel_select
    it was built for, so that the GPU comparison below is a comparison ON those paths.

    What the output can show of cal_exp_tim: every inside candidate of an agent carries the same 1 / tc_min (it is a
    property of the agent's state, not of the candidate), so the penalty minimum is the distance minimum unless tc_min
    is 0 (penalty inf for all: the first inside candidate wins) - the output tells whether tc_min is 0, infinite or
    finite, never its finite value.  No scene can test more than that, and none tries."""
    sc, run = SCENES[k], scene_oracle(k)
    c = run.counts()
    print(sc.label, run.tally_extra(), "knife", int((run.margin < 1e-9).sum()))
    assert sum(c[b] for b in (OUT_ONLY, OUT_SOME_IN, IN_ONLY, NONE)) == sc.E * sc.N
    for what, least in sc.floors.items():
        assert c[what] >= least, (sc.label, what, c)
    if sc.only is not None:
        assert c[sc.only] == sc.E * sc.N, (sc.label, c)
    if sc.only == NONE:
        assert not run.want.any()
    assert (run.want[run.branch == NONE] == 0).all()
    live = run.branch != NONE
    assert (np.linalg.norm(run.want[live], axis=-1) >= 0.3).all()       # vel_candidate's own gate on every winner
    assert int((run.margin < 1e-9).sum()) <= knife_bound(sc.E * sc.N)


def test_scene_table_covers_every_path_and_flag():
    """Every code and both flags are well populated somewhere; codes 1 and 2 also beyond four waves (N > 256); mask bit
    63 is in use (64 live candidates) where acceler is 1; the per-drone priorities are visible in the output."""
    tot, wide = collections.Counter(), collections.Counter()
    for k, sc in enumerate(SCENES):
        c = scene_oracle(k).counts()
        tot.update(c)
        if sc.N > 256:
            wide.update(c)
    assert all(tot[b] >= 100 for b in (OUT_ONLY, OUT_SOME_IN, IN_ONLY, NONE, OVERLAP, TC_ZERO)), tot
    assert wide[OUT_SOME_IN] >= 100 and wide[IN_ONLY] >= 100, wide
    assert {sc.N for sc in SCENES if sc.N > 256} == {300, 512}          # five and eight waves, the last partly filled / full
    k8 = SCENE_IDS.index("eight_waves")
    _, _, vel, _, _ = scene_state(k8)
    n64 = sum(len(orc.rvo_candidates(v, SCENES[k8].vmax, 1.0)) == 64 for v in vel[0])
    assert n64 >= 20, n64
    kp = SCENE_IDS.index("dense_per_drone")
    differ = (scene_oracle(kp).want != scene_oracle(kp, True).want).any(axis=-1)
    assert int(differ.sum()) >= 100, int(differ.sum())


# A candidate that only the reference's own sequence decides: pairs of drones 3 m apart along a grid velocity, with
# opposite velocities and equal priorities, so that PAA = pr (2 p + va + vb) is the drone's own position and the
# candidate pointing at the neighbour has cs = 1 up to the rounding of the norms - on either side of 1.  arccos of
# 1 + ulp is NaN, beta NaN, alpha > beta false: outside; cs <= 1: beta 0, inside.
EDGE_DIRS = [(0.5, 0.0, 0.0), (1.0, 0.0, 0.0), (0.5, 0.5, 0.0), (1.0, 0.5, 0.5), (0.5, -1.0, 0.5), (1.0, -0.5, -1.0),
             (-0.5, 0.5, 0.5), (0.5, 0.5, 0.5)]
EDGE_E, EDGE_ACCELER = 32, 1.0


@functools.lru_cache(maxsize=None)
def edge_state():
    from rvo3d_amd import synthetic_world
    rng = np.random.default_rng(23)
    w = synthetic_world(EDGE_E, 2, (8.0, 8.0, 8.0), seed=int(rng.integers(1 << 30)), min_sep=0.5)
    pos, vel = np.empty((EDGE_E, 2, 3)), np.empty((EDGE_E, 2, 3))
    for e in range(EDGE_E):
        d = np.array(EDGE_DIRS[e % len(EDGE_DIRS)])
        pos[e, 0] = (3.0, 2.0, 3.0) if e == 0 else rng.uniform(2.0, 6.0, 3)   # env 0: the plain case, +x at equal height
        pos[e, 1] = pos[e, 0] + 3.0 * d / np.linalg.norm(d)
        vel[e, 0] = (0.5, 0.0, 0.0)                                           # every direction above is on its grid
        vel[e, 1] = -vel[e, 0]
    return w, pos, vel, None, None


@functools.lru_cache(maxsize=None)
def edge_oracle():
    return OracleRun(*edge_state(), V2, EDGE_ACCELER)


def test_edge_scene_puts_a_candidate_on_cs_equal_one():
    run = edge_oracle()
    vel = edge_state()[2]
    for e in range(EDGE_E):                                                # the candidate is on the drone's grid
        d = np.array(EDGE_DIRS[e % len(EDGE_DIRS)])
        assert (orc.rvo_candidates(vel[e, 0], V2, EDGE_ACCELER) == d).all(axis=1).any(), e
    cs = run.cs_near_one[:, 0]
    print("cs - 1 of drone 0:", (cs - 1).tolist())
    assert (np.abs(cs - 1) <= 1e-9).all()
    assert (cs > 1).sum() >= 3 and (cs <= 1).sum() >= 3                       # both sides of arccos' domain edge
    assert cs[0] == 1.0
    assert int((run.margin < 1e-9).sum()) <= knife_bound(2 * EDGE_E)


def _gpu_compare(name, state, run, vmax, acceler):
    """env.rvo_vel against the oracle's run of the same state with the knife-edge accounting of the step tests, and what
    else a call owes its caller: des_vel equal, the state untouched, nothing written outside [E, N, 3], the same bits twice."""
    import ctypes as C
    import torch
    from rvo3d_amd import BatchedDroneEnv, _lib
    from test_gpu_parity import Tally
    w, pos, vel, radius, priority = state
    E, N = pos.shape[:2]
    env = BatchedDroneEnv(w, neighbors_num=10, radius=radius, priority=priority)
    try:
        env.set_state(pos=pos, vel=vel)
        np.testing.assert_array_equal(env.des_vel().cpu().numpy(), run.des)   # (orc_des_vel leaves no margins)
        before = {k: v.cpu().numpy().copy() for k, v in env.get_state().items()}
        got = env.rvo_vel(vmax, acceler).cpu().numpy()
        tl = Tally(name, E)
        tl.begin(run.margin)
        tl.check("rvo_vel", got == run.want)
        tl.end()
        rec = tl.finish(**run.tally_extra())
        print(name, rec)
        after = env.get_state()
        assert set(after) == set(before) and len(before) == 10
        for k in before:
            np.testing.assert_array_equal(after[k].cpu().numpy(), before[k], err_msg=k)
        # second call, into a view of a larger buffer: the rows before and behind keep the sentinel
        pad, sentinel = 192, -777.25
        big = torch.full((pad + E * N + pad, 3), sentinel, dtype=torch.float64, device=env.device)
        out = big[pad:pad + E * N]
        vm = (C.c_double * 3)(*vmax)
        _lib.check(_lib.lib().rvo3d_rvo_vel(env._h, vm, float(acceler), C.c_void_p(out.data_ptr()), env._stream()),
                   "rvo3d_rvo_vel")
        torch.cuda.synchronize()
        host = big.cpu().numpy()
        assert (host[:pad] == sentinel).all() and (host[pad + E * N:] == sentinel).all()
        assert host[pad:pad + E * N].tobytes() == got.tobytes()
    finally:
        env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(SCENES)), ids=SCENE_IDS)
def test_hip_rvo_vel_matches_oracle_on_scene(k):
    sc = SCENES[k]
    _gpu_compare(f"rvo_vel/{sc.label}", scene_state(k), scene_oracle(k), sc.vmax, sc.acceler)


@pytest.mark.gpu
def test_hip_rvo_vel_matches_oracle_where_cs_is_one():
    """The kernel's cosine-threshold shortcut must hand these candidates to the reference's own sequence (cs within
    1e-9 of 1): whether arccos sees 1, 1 - ulp or 1 + ulp (NaN: outside) is decided by the roundings of that sequence."""
    _gpu_compare("rvo_vel/cs_is_one", edge_state(), edge_oracle(), V2, EDGE_ACCELER)


def _city_drone_side_cases():
    """The cs = 1 edge scene, eight_waves (64 live candidates: mask bit 63) and the smallest scene of the table whose
    floors include IN_ONLY."""
    with_in_only = [k for k, sc in enumerate(SCENES) if IN_ONLY in sc.floors]
    small = min(with_in_only, key=lambda k: SCENES[k].E * SCENES[k].N)
    k8 = SCENE_IDS.index("eight_waves")
    assert small != k8
    return [("cs_is_one", None), ("eight_waves", k8), (SCENES[small].label, small)]


@pytest.mark.gpu
@pytest.mark.parametrize("label,k", _city_drone_side_cases(), ids=[c[0] for c in _city_drone_side_cases()])
def test_hip_rvo_vel_city_drone_side_is_rvo_vel_on_the_pinned_states(label, k):
    """rvo_vel_city with a reach no building is within (1e-300) on the states the oracle pins for rvo_vel: the row is
    rvo_vel's bit for bit, nothing is gated or blocked, and the tier is the oracle's branch - 1 for a winner outside
    every cone, 2 for one inside, 4 for no live candidate - for every agent further than 1e-9 from a rounding tie;
    those nearer are at most knife_bound of them."""
    import torch
    from rvo3d_amd import BatchedDroneEnv
    if k is None:
        state, run, vmax, acceler = edge_state(), edge_oracle(), V2, EDGE_ACCELER
    else:
        state, run, vmax, acceler = scene_state(k), scene_oracle(k), SCENES[k].vmax, SCENES[k].acceler
    w, pos, vel, radius, priority = state
    E, N = pos.shape[:2]
    env = BatchedDroneEnv(w, neighbors_num=10, radius=radius, priority=priority)
    try:
        env.set_state(pos=pos, vel=vel)
        plain = env.rvo_vel(vmax, acceler)
        city, diag = env.rvo_vel_city(diagnostics=True, vmax=vmax, acceler=acceler, reach=1e-300)
        torch.cuda.synchronize()
        assert torch.equal(city.view(torch.int64), plain.view(torch.int64))
        d = {n: t.cpu().numpy() for n, t in diag.items()}
    finally:
        env.close()
    assert not d["n_gated"].any()
    assert not d["blocked_mask"].any()
    if label == "eight_waves":
        assert (d["live_mask"] < 0).any()                                     # bit 63 of the int64 view
    sure = run.margin >= 1e-9
    print(label, "agents", E * N, "within 1e-9 of a tie", int((~sure).sum()),
          "tiers", {t: int((d["tier"] == t).sum()) for t in (0, 1, 2, 3, 4)})
    assert int((~sure).sum()) <= knife_bound(E * N)
    want = np.zeros((E, N), np.int32)
    want[(run.branch == OUT_ONLY) | (run.branch == OUT_SOME_IN)] = 1
    want[run.branch == IN_ONLY] = 2
    want[run.branch == NONE] = 4
    assert (want > 0).all()
    assert (d["tier"][sure] == want[sure]).all(), np.argwhere(sure & (d["tier"] != want))[:10]


@pytest.mark.gpu
def test_hip_rvo_vel_rejects_bad_arguments_and_writes_nothing():
    import ctypes as C
    import torch
    from rvo3d_amd import BatchedDroneEnv, _lib
    k = SCENE_IDS.index("slow")
    w, pos, vel, _, _ = scene_state(k)
    env = BatchedDroneEnv(w, neighbors_num=10)
    try:
        env.set_state(pos=pos, vel=vel)
        L, invalid = _lib.lib(), -1                                           # RVO3D_ERR_INVALID (include/rvo3d.h)
        out = torch.full((env.E, env.N, 3), -777.25, dtype=torch.float64, device=env.device)
        vm, po = (C.c_double * 3)(2.0, 2.0, 2.0), C.c_void_p(out.data_ptr())
        for acc in (-1e-12, float(np.nextafter(1.0, 2.0)), float("nan"), float("inf"), -float("inf")):
            assert L.rvo3d_rvo_vel(env._h, vm, acc, po, env._stream()) == invalid, acc
            assert b"acceler" in L.rvo3d_last_error()
        assert L.rvo3d_rvo_vel(env._h, None, 0.5, po, env._stream()) == invalid
        assert L.rvo3d_rvo_vel(env._h, vm, 0.5, None, env._stream()) == invalid
        assert L.rvo3d_rvo_vel(None, vm, 0.5, po, None) != 0
        torch.cuda.synchronize()
        assert bool((out == -777.25).all())
        # the two ends of the accepted range are accepted
        for acc in (0.0, 1.0):
            assert L.rvo3d_rvo_vel(env._h, vm, acc, po, env._stream()) == 0
        torch.cuda.synchronize()
        assert not bool((out == -777.25).any())
    finally:
        env.close()
