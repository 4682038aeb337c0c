"""The policy-step kernels' launch geometry and the error model at the env's own scale, on the host.

Every policy-step kernel launches a fixed grid and loops over its work inside the kernel ("trips").  trip_sizes(cus) is
the table tests/test_gpu_policy_trips.py sizes its launches from - rows or tiles one trip of each kernel covers on a
device with `cus` compute units -, and test_launch_geometry_is_what_the_trip_sizes_assume pins the facts of the sources
it is computed from: if that test fails, the geometry changed - update trip_sizes() (and nothing else) to match.

test_error_model_at_env_scale is tests/test_rnn_x3_host.py's emulation of the split-bf16 products on rows at the env's
scale (positions up to 50, every row with VO rows): the reference alone leaves the bounds MU_MAX / MU_MEAN / V_REL a
30x margin there (mu max 2.9e-6 / 2.7e-6, v max 2.8e-6 / 2.5e-6 for (256, biGRU) / (64, GRU); bf16 stacks 1.6e-3), so
the GPU test on these rows may use the same bounds."""
import collections
import os
import re

import pytest
import torch

from conftest import PKG_DIR
from test_policy_x3_host import MU_MAX, MU_MEAN, V_REL, config3_like_obs
from test_rnn_x3_host import _ac, _inside, emulate_rows, forward64, mm_bf16, mm_x3

TripSizes = collections.namedtuple("TripSizes", "tiles_per_trip bucket_rows_per_pass mlp_rows_per_trip reader_rows_per_trip")

# the facts of the sources the table rests on (test_launch_geometry_is_what_the_trip_sizes_assume reads them back)
RNN_TILES_WAVES = 4          # kRnnTilesWaves: waves per workgroup, one 32-row tile each; the grid is one workgroup per CU
BUCKET_GRID, BUCKET_BLOCK = 256, 256   # rnn_tiles_bucket_kernel: dim3(256), dim3(256), one list entry per thread and pass
MLP_WAVES, MLP_ROWS_PER_WAVE = 8, 64   # RVO3D_MLP_WAVES; a wave finishes 64 rows (two 32-row passes) per trip
READER_GRID_CAP, READER_ROWS = 256 * 8, 8   # reader_first_step_kernel: at most 256 * 8 workgroups of kReaderRows rows


def trip_sizes(cus):
    """What one trip of each policy-step kernel covers on a device with `cus` compute units."""
    return TripSizes(
        tiles_per_trip=RNN_TILES_WAVES * max(cus, 1),                                  # "nw": 32-row tiles
        bucket_rows_per_pass=BUCKET_GRID * BUCKET_BLOCK,                               # listed rows
        mlp_rows_per_trip=(cus // 2 if cus >= 2 else 1) * MLP_WAVES * MLP_ROWS_PER_WAVE,   # rows per network
        reader_rows_per_trip=READER_GRID_CAP * READER_ROWS)                            # rows


def _src(name):
    with open(os.path.join(PKG_DIR, "csrc", name)) as f:
        return f.read()


def _has(text, pattern):
    return re.search(pattern, text) is not None


def test_launch_geometry_is_what_the_trip_sizes_assume():
    """A failure here means the launch geometry changed: update trip_sizes() in this file, the GPU tests follow."""
    capi, tiles, rollout, mlp = (_src(n) for n in ("rvo3d_capi.hip", "rvo3d_policy_rnn_tiles.hpp",
                                                   "rvo3d_rollout_kernels.hpp", "rvo3d_policy_mlp.hpp"))
    hint = "the launch geometry changed: update trip_sizes() in tests/test_policy_trips_host.py"
    # tiles: one workgroup of kRnnTilesWaves waves per CU; a wave takes tiles gw, gw + nw, ...
    assert _has(tiles, r"constexpr int kRnnTilesWaves = %d;" % RNN_TILES_WAVES), hint
    assert _has(capi, r"const unsigned grid = \(unsigned\)\(cus > 0 \? cus : 1\);"), hint
    assert _has(capi, r"policy_rnn_tiles_kernel<H, ND, X3>\), dim3\(grid\), dim3\(64 \* rvo3d::kRnnTilesWaves\)"), hint
    assert _has(tiles, r"gw = blockIdx\.x \* kRnnTilesWaves \+ wave, nw = gridDim\.x \* kRnnTilesWaves;"), hint
    assert _has(tiles, r"for \(int tile = gw; tile < total; tile \+= nw\)"), hint
    # the bucket kernel: 256 x 256 threads, grid-strided, one list entry per thread
    assert _has(capi, r"rnn_tiles_bucket_kernel, dim3\(%d\), dim3\(%d\)," % (BUCKET_GRID, BUCKET_BLOCK)), hint
    assert _has(tiles, r"i0 = \(int64_t\)blockIdx\.x \* 256 \+ \(threadIdx\.x & ~63\); i0 < n_use; "
                       r"i0 \+= \(int64_t\)gridDim\.x \* 256\)"), hint
    # the MLP kernels: G = min(chunks / waves, cus / 2) workgroups per network, 64 rows per wave and trip
    assert _has(capi, r"#define RVO3D_MLP_WAVES %d\b" % MLP_WAVES), hint
    assert _has(capi, r"constexpr int kMlpWaves = RVO3D_MLP_WAVES;"), hint
    assert _has(capi, r"const int64_t nchunks = \(rows \+ 63\) / 64;"), hint
    assert _has(capi, r"const int64_t Gmax = cus >= 2 \? cus / 2 : 1;"), hint
    assert _has(capi, r"const unsigned grid = \(unsigned\)\(2 \* G\);"), hint
    assert _has(capi, r"dim3\(grid\), dim3\(64 \* kMlpWaves\)"), hint
    assert _has(mlp, r"return \(int64_t\)g \* NW \+ wave \+ \(int64_t\)\(pass >> 1\) \* G \* NW;"), hint
    # the reader: at most 256 * 8 workgroups, kReaderRows rows each per trip
    assert _has(rollout, r"constexpr int kReaderRows = %d;" % READER_ROWS), hint
    assert _has(capi, r"const unsigned grid = \(unsigned\)\(groups < 256 \* 8 \? groups : 256 \* 8\);"), hint
    assert _has(rollout, r"for \(int64_t grp = blockIdx\.x; grp < ngroups; grp \+= gridDim\.x\)"), hint
    assert READER_GRID_CAP == 256 * 8
    # the table on the 256-CU MI355X, and on small or odd devices
    assert trip_sizes(256) == (1024, 65536, 65536, 16384)
    assert trip_sizes(1) == (4, 65536, 512, 16384) and trip_sizes(5) == (20, 65536, 1024, 16384)
    # a chunk of 16 nw listed rows fills at most nw tiles whatever its counts: every count's last tile may be ragged
    for cus in (8, 64, 256, 304):
        nw = trip_sizes(cus).tiles_per_trip
        assert 16 * nw <= 32 * (nw - 12)


@pytest.mark.parametrize("hidden,bi", [(256, True), (64, False)])
def test_error_model_at_env_scale(hidden, bi):
    """emulate_rows with every product split stays inside MU_MAX / MU_MEAN / V_REL against float64 on config-3-like rows
    that all carry VO rows (counts 1..12, positions up to 50); with bf16 stacks it falls outside."""
    ac = _ac(hidden, bi, 5 + hidden + bi)
    obs, cnt = config3_like_obs(1536, 12 + 9 * 12, vo_share=1.0, seed=3)
    cnt = cnt.to(torch.int64)
    assert int(cnt.min()) >= 1 and sorted(set(cnt.tolist())) == list(range(1, 13))
    assert float(obs[:, :12].abs().max()) > 40.0 and float(obs[:, 12:].abs().max()) > 40.0
    with torch.no_grad():
        z64, v64 = forward64(ac, obs, cnt)
        ok3, fig3 = _inside(*emulate_rows(ac, obs, cnt, mm_x3, mm_x3), z64, v64)
        okb, figb = _inside(*emulate_rows(ac, obs, cnt, mm_x3, mm_bf16), z64, v64)
    print(f"hidden {hidden} bi {bi}: x3 mu max {fig3[0]:.2e} mean {fig3[1]:.2e} v max {fig3[2]:.2e}; "
          f"bf16 stacks mu max {figb[0]:.2e} mean {figb[1]:.2e} v max {figb[2]:.2e}")
    assert ok3, fig3
    assert fig3[0] <= MU_MAX and fig3[1] <= MU_MEAN and fig3[2] <= V_REL * float(v64.abs().clamp(min=1.0).max())
    assert not okb and figb[0] > MU_MAX and figb[1] > MU_MEAN, figb
