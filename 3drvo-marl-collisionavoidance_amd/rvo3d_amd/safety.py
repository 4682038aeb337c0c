"""Safety metrics of an evaluation: the plain numpy restatement of rvo3d_safety_scan's rules (include/rvo3d.h) that the
tests compare the kernel against, and the summary of the evaluator's safety records.  No GPU needed."""
from __future__ import annotations

import numpy as np


def _fold_min(cands, out):
    """The header's minimum rule over the rows of cands: from `out` (+inf), x < m ? x : m."""
    for x in cands:
        out = np.where(x < out, x, out)
    return out


def safety_numpy(pos, radius, map_size, near_margin, counts=None, buildings=None, building_counts=None):
    """rvo3d_safety_scan in numpy, rule by rule and operation by operation (float64, every product and sum on its own).
    pos [E, N, 3], radius [E, N] (or anything that broadcasts to it), map_size [3], counts [E] or None (every env has N
    live drones), buildings [nb, 4] shared or [E, nb_max, 4] per env (x, y, h, r) with building_counts [E] or None (all
    nb_max), or None.  Returns (sep [E, N], bclear [E, N], wall [E, N] float64 with +inf in the ghost rows, near_pairs [E]
    int32).  Ghost rows of pos / radius are never read."""
    pos = np.asarray(pos, dtype=np.float64)
    E, N, _ = pos.shape
    radius = np.broadcast_to(np.asarray(radius, dtype=np.float64), (E, N))
    ms = np.asarray(map_size, dtype=np.float64)
    sep, bclear, wall = (np.full((E, N), np.inf) for _ in range(3))
    near = np.zeros(E, dtype=np.int32)
    bld = None if buildings is None else np.asarray(buildings, dtype=np.float64)
    for e in range(E):
        n = N if counts is None else int(counts[e])
        p, r = pos[e, :n], radius[e, :n]
        # 1. / 4.: rel = p_j - p_i, dis = sqrt((rel_y^2 + rel_x^2) + rel_z^2), d = dis - (r_i + r_j)
        rel = p[None, :, :] - p[:, None, :]                       # [i, j]
        rx, ry, rz = rel[..., 0], rel[..., 1], rel[..., 2]
        d = np.sqrt((ry * ry + rx * rx) + rz * rz) - (r[:, None] + r[None, :])
        other = ~np.eye(n, dtype=bool)
        sep[e, :n] = _fold_min([np.where(other[:, j], d[:, j], np.inf) for j in range(n)], np.full(n, np.inf))
        near[e] = int(np.count_nonzero(np.triu(d <= near_margin, 1)))
        # 2.: the buildings the env collides with, those with p_z <= h
        if bld is not None and bld.size:
            if bld.ndim == 3:
                nb = bld.shape[1] if building_counts is None else int(building_counts[e])
                B = bld[e, :nb]
            else:
                B = bld.reshape(-1, 4)
            ex, ey = p[:, 0:1] - B[None, :, 0], p[:, 1:2] - B[None, :, 1]
            c = np.sqrt(ex * ex + ey * ey) - (r[:, None] + B[None, :, 3])
            c = np.where(p[:, 2:3] <= B[None, :, 2], c, np.inf)
            bclear[e, :n] = _fold_min([c[:, b] for b in range(B.shape[0])], np.full(n, np.inf))
        # 3.: the six faces, + 0.0
        cands = []
        for k in range(3):
            cands += [p[:, k], ms[k] - p[:, k]]
        wall[e, :n] = _fold_min(cands, np.full(n, np.inf)) + 0.0
    return sep, bclear, wall, near


def fold_safety_step(run, sep, bclear, wall, near_pairs):
    """One step of the episode fold (rvo3d_eval_account_safety) on the host: run = dict(sep, bclear, wall [E] float64,
    near [E] int64), updated in place with the per-env minima of this step's scan outputs (ghost rows are +inf) and its
    near_pairs.  Returns run."""
    for k, v in (("sep", sep), ("bclear", bclear), ("wall", wall)):
        step = np.min(np.asarray(v, dtype=np.float64), axis=1)
        run[k] = np.where(step < run[k], step, run[k])
    run["near"] = run["near"] + np.asarray(near_pairs, dtype=np.int64)
    return run


def new_safety_run(E):
    """The running values at the start of an episode: +inf, +inf, +inf, 0."""
    return dict(sep=np.full(E, np.inf), bclear=np.full(E, np.inf), wall=np.full(E, np.inf), near=np.zeros(E, np.int64))


def summarize_safety(min_sep, min_bclear, min_wall, near, length, drones):
    """The evaluation's safety figures from its episode records (one entry per counted episode, any order): min_sep,
    min_bclear, min_wall - the per-episode minima (+inf: the episode never had a second drone / a building that
    counts) -, near - the episode's near-miss pair-steps -, length - its steps -, drones - the drones of its env (a
    number or one per episode).  Means are over the episodes whose minimum is finite (nan when there is none)."""
    near = np.asarray(near, dtype=np.int64).reshape(-1)
    length = np.asarray(length, dtype=np.int64).reshape(-1)
    drones = np.broadcast_to(np.asarray(drones, dtype=np.int64), length.shape)
    out = {}
    for name, v in (("sep", min_sep), ("bclear", min_bclear), ("wall", min_wall)):
        v = np.asarray(v, dtype=np.float64).reshape(-1)
        fin = v[np.isfinite(v)]
        out[f"mean_min_{name}"] = float(np.mean(fin)) if fin.size else float("nan")
        out[f"min_min_{name}"] = float(np.min(v)) if v.size else float("inf")
    drone_steps = int(np.sum(length * drones))
    out["near_per_1000_drone_steps"] = 1000.0 * float(np.sum(near)) / drone_steps if drone_steps else 0.0
    out["near_episode_share"] = float(np.mean(near > 0)) if near.size else 0.0
    out["episodes"] = int(near.size)
    return out
