"""The moving buildings' rules in numpy float64 (include/rvo3d.h: rvo3d_move_env_buildings), for the tests: one numpy
ufunc per operation, so every operation is rounded on its own, and np.sqrt / np.divide are correctly rounded."""
import numpy as np

CELL = 8.0  # the cell size of the lists on maps up to 512 m


def move(bld, ends, speed, leg, dt, env_mask=None):
    """One time step.  bld [E, nb, 4], ends [E, nb, 2, 2], speed [E, nb], leg [E, nb] uint8 -> (bld, leg), new arrays."""
    bld = np.array(bld, dtype=np.float64)
    leg = np.array(leg, dtype=np.uint8)
    x, y, h = bld[..., 0], bld[..., 1], bld[..., 2]
    step = np.asarray(speed, dtype=np.float64) * np.float64(dt)
    with np.errstate(all="ignore"):
        mv = ~(h == -np.inf) & (step > 0)
        if env_mask is not None:
            mv &= np.asarray(env_mask).astype(bool)[:, None]
        k = (leg & 1).astype(np.int64)
        T = np.take_along_axis(np.asarray(ends, dtype=np.float64), k[..., None, None], axis=-2)[..., 0, :]
        dx, dy = T[..., 0] - x, T[..., 1] - y
        d = np.sqrt(dx * dx + dy * dy)
        arrive = mv & (d <= step)
        go = mv & ~arrive
        nx, ny = x + (dx / d) * step, y + (dy / d) * step
    out = bld.copy()
    out[..., 0] = np.where(arrive, T[..., 0], np.where(go, nx, x))
    out[..., 1] = np.where(arrive, T[..., 1], np.where(go, ny, y))
    return out, np.where(arrive, leg ^ 1, leg).astype(np.uint8)


def cell_of(x, y, nx, ny, cs=CELL):
    """The cell the step looks a position up in: floor, clamped."""
    ix = np.clip(np.floor(np.asarray(x) / cs), 0, nx - 1).astype(np.int64)
    iy = np.clip(np.floor(np.asarray(y) / cs), 0, ny - 1).astype(np.int64)
    return ix * ny + iy


def list_lengths(b, rmax, nx, ny, cs=CELL):
    """How many of the buildings b [n, 4] each cell lists, by brute force ([nx * ny]; more than 15 overflows)."""
    out = np.zeros(nx * ny, np.int64)
    for ix in range(nx):
        for iy in range(ny):
            x0, x1 = (-np.inf if ix == 0 else ix * cs), (np.inf if ix == nx - 1 else (ix + 1) * cs)
            y0, y1 = (-np.inf if iy == 0 else iy * cs), (np.inf if iy == ny - 1 else (iy + 1) * cs)
            dx = np.where(b[:, 0] < x0, x0 - b[:, 0], np.where(b[:, 0] > x1, b[:, 0] - x1, 0.0))
            dy = np.where(b[:, 1] < y0, y0 - b[:, 1], np.where(b[:, 1] > y1, b[:, 1] - y1, 0.0))
            reach = np.minimum(rmax + b[:, 3], 5.0) + 1e-3
            out[ix * ny + iy] = int((dx * dx + dy * dy <= reach * reach).sum())
    return out
