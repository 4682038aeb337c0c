"""The inputs of tests/test_gpu_filter_edges.py, checked on the CPU with the oracle alone (tests/filter_edge_cases.py).

For every (shape, map, config) and every (mode, bucket) of it:
  * at least 40 constructed pairs lie on each side of the decision surface;
  * the oracle answers what the construction says - the row of i exists on one side only, `done` / the "math domain
    error" count follow the touch surfaces - so a filter that drops or keeps the wrong pairs changes an output;
  * the samples with an oracle margin below 1e-9 stay within the cap of test_gpu_parity.Tally.finish
    (1 % + 3 sigma + 2); apart from the 1e-12 m/s drones of the approach rounds, which are such samples on purpose,
    there is at most one per bucket;
  * the same decision taken in float32 WITHOUT any error band (centred coordinates cast to float32, fma-order sums)
    misreads at least 20 of the pairs on the maps of 500 m and more: the inputs are inside the float32 noise.  The
    20 m control is exempt; its count is printed.
"""
import numpy as np
import pytest

import filter_edge_cases as fe

KNIFE = 1e-9
CASES = [(s, m, c) for s in fe.SHAPES for m in fe.MAPS for c in fe.CONFIGS if c != "reset"]
RESET_CASES = [(s, m) for s in fe.SHAPES for m in fe.MAPS if m != fe.CONTROL]


@pytest.mark.parametrize("shape,map_name,config", CASES)
def test_constructed_pairs_decide_the_oracles_output(shape, map_name, config):
    case = fe.Case(shape, map_name, config)
    ref = fe.RefBatch(case)
    E, N = case.E, case.N
    live = np.arange(N)[None, :] < np.asarray(case.live)[:, None]
    stats = {}
    for rd in case.rounds:
        st = stats.setdefault((rd.mode, rd.bucket), dict(side=[0, 0], samples=0, knife=0, planned_knife=0, misread=0,
                                                         rows=[0, 0], done=[0, 0], autoreset=set(), unclaimed_rows=0, stray_knife=0,
                                                         domain=[0, 0]))
        ref.set_state(**case.full_state(rd))
        dom0 = ref.domain_count
        if rd.mode == "observe":
            obs, cnt = ref.observe()
            done = rm = None
        else:
            obs, cnt, rew, done, info, fin, rm = ref.step(rd.actions, rd.autoreset)
            assert not fin.any() and not info.any()
            st["autoreset"].add(rd.autoreset)
        mg = ref.margin()
        assert np.isfinite(obs).all()
        # what the construction claims
        post = ref.get_state()["pos"] if (rd.mode == "step" and not rd.autoreset) else None
        claimed = rd.expect_rows >= 0
        env_ok = np.ones(E, bool)
        if rm is not None:
            env_ok = ~rm.astype(bool).any(axis=1)  # (an env that reset somebody was observed again, at rest)
        chk = claimed & live & env_ok[:, None]
        assert (cnt[chk] == rd.expect_rows[chk]).all(), (rd.mode, rd.bucket, rd.where, np.argwhere(chk & (cnt != rd.expect_rows))[:5])
        if done is not None:
            out = np.zeros((E, N), bool)
            out[rd.env, rd.i] = case.outside_map(rd.xi)
            out[rd.env, rd.j] = case.outside_map(rd.xj)
            want = (rd.expect_done != 0) | out
            assert (done.astype(bool)[live] == want[live]).all(), (rd.mode, rd.bucket, rd.where)
            if not case.small:
                assert not out.any()  # on the large maps the step rounds stay inside the map
        dom = ref.domain_count - dom0
        assert (dom > 0) == rd.expect_domain, (rd.bucket, dom)
        st["domain"][int(dom > 0)] += 1
        if post is not None:  # the move ended where the construction put it
            assert np.abs(post[rd.env, rd.i] - rd.xi).max() <= 4e-16 * max(case.map_size) * 4
        # the accounting
        cl = rd.claim
        st["side"][0] += int((~rd.side & cl).sum()); st["side"][1] += int((rd.side & cl).sum())
        ei = env_ok[rd.env] & cl
        for s in (0, 1):
            sel = ei & (rd.side == bool(s))
            st["rows"][s] += int(cnt[rd.env[sel], rd.i[sel]].sum())
            if done is not None:
                st["done"][s] += int(done[rd.env[sel], rd.i[sel]].sum())
        st["unclaimed_rows"] += int(cnt[rd.env[~cl], rd.i[~cl]].sum())
        planned = np.zeros((E, N), bool)
        if rd.bucket == "approach":
            k3 = rd.kind == 3
            planned[rd.env[k3], rd.i[k3]] = True
        st["samples"] += int(live.sum())
        st["knife"] += int((mg[live] < KNIFE).sum())
        st["planned_knife"] += int(planned.sum())
        st["stray_knife"] += int(((mg < KNIFE) & live & ~planned).sum())
        st["misread"] += int((fe.naive_f32_side(case, rd) != rd.side)[cl].sum())
    assert set(stats) == set(case.plan)
    for (mode, bucket), st in stats.items():
        print(f"{shape} {map_name} {config} {mode}/{bucket}: {st}")
        assert min(st["side"]) >= fe.PER_SIDE, (mode, bucket, st)
        lim = 0.01 * st["samples"]
        assert st["knife"] <= lim + 3.0 * np.sqrt(lim) + 2, (mode, bucket, st)
        assert st["stray_knife"] <= 1, (mode, bucket, st)  # (an observation value next to a rounding tie: one in 1e5)
        # both sides change an output
        if bucket == "touch_eval":
            assert st["done"][0] > 0 and st["rows"] == [0, 0], st
            if not case.small:
                assert st["done"][1] == 0, st
        else:
            assert st["rows"][0] == 0 and st["rows"][1] >= fe.PER_SIDE // 2, (mode, bucket, st)
            if bucket == "touch" and not case.small:
                assert st["done"][0] >= fe.PER_SIDE // 2 and st["done"][1] == 0, st
        if bucket == "domain":
            assert st["domain"][0] > 0 and st["domain"][1] > 0, st
        if mode == "step":
            assert st["autoreset"] == {False, True}, st
        if map_name != fe.CONTROL:
            assert st["misread"] >= 20, (mode, bucket, st)
    if config == "radii" and not case.small:
        assert stats[("observe", "cone")]["unclaimed_rows"] > 0  # unequal priorities: rows the filter must not drop


@pytest.mark.parametrize("shape,map_name", RESET_CASES)
def test_reset_rounds_decide_the_second_steps_flag(shape, map_name):
    """The partner is reset by the first step and nobody else is; in the state the first step leaves, the oracle
    flags i under the second step's action exactly on the constructed side."""
    case = fe.Case(shape, map_name, "reset")
    ref = fe.RefBatch(case)
    live = np.arange(case.N)[None, :] < np.asarray(case.live)[:, None]
    side, kinds, misread, knife, samples, autoreset = [0, 0], [0, 0], 0, 0, 0, set()
    for rd in case.rounds:
        ref.set_state(**case.full_state(rd))
        rm = ref.step(rd.actions, True)[6].astype(bool)
        want = np.zeros_like(rm)
        want[rd.env, rd.j] = True
        assert (rm == want).all()
        knife += int((ref.margin()[live] < KNIFE).sum())
        flag = np.array([ref.vo_flag(e, i, rd.actions2[e, i]) for e, i in zip(rd.env, rd.i)])
        assert (flag == rd.side).all(), np.flatnonzero(flag != rd.side)[:5]
        np.testing.assert_array_equal(ref.get_state()["pos"][rd.env, rd.j], rd.xj)
        ref.step(rd.actions2, rd.autoreset)
        knife += int((ref.margin()[live] < KNIFE).sum())
        samples += 2 * int(live.sum())
        autoreset.add(rd.autoreset)
        side[0] += int((~rd.side).sum()); side[1] += int(rd.side.sum())
        for k in (0, 1):
            kinds[k] += int((rd.kind == k).sum())
        misread += int((fe.naive_f32_side(case, rd) != rd.side).sum())
    print(f"{shape} {map_name} reset: side {side} gate/touch {kinds} misread {misread} knife {knife} of {samples}")
    assert min(side) >= fe.PER_SIDE and min(kinds) >= fe.PER_SIDE // 2 and autoreset == {False, True}
    lim = 0.01 * samples
    assert knife <= lim + 3.0 * np.sqrt(lim) + 2
    assert misread >= 20
