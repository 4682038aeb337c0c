"""The policy-step kernels beyond one grid trip, and the tiles entry points at the edges of their documented contract.

Every policy-step kernel launches a fixed grid and loops over its work inside the kernel.  The sizes below come from
tests/test_policy_trips_host.py::trip_sizes(CUs) (pinned against the sources there), so each launch provably spans
more than two trips - and the bucket kernel more than one pass - on the device the test runs on; the tests assert it.
Two references throughout: a float64 forward of the modules within the bounds the project already has (MU_MAX /
MU_MEAN / V_REL for the float32-class kernels, 3e-2 for the bf16 ones, 3e-5 for the reader), and THE SAME ROWS COMPUTED
ONE TRIP AT A TIME, bit for bit - whatever a wave carries from one trip to the next (LDS state, accumulators, the
fragment ring, the opaque blob pointer) shows up there.

  2a  policy_rnn_tiles_kernel<H, ND, X3> + rnn_tiles_bucket_kernel   test_tiles_span_several_trips
  2b  policy_mlp_x3_kernel, policy_mlp_kernel at W = 39                test_mlp_spans_several_trips
  2c  reader_first_step_kernel                                         test_reader_first_step_spans_several_trips
  2d  include/rvo3d.h's contract of the tiles entry points             test_tiles_*  (small shapes)
  2e  accuracy at the env's own scale (positions up to 50)             test_tiles_accuracy_at_env_scale

Measured on an MI355X (256 CUs: nw = 1024 tiles, 65 536 rows per bucket pass and per MLP trip, 16 384 per reader
trip), error against float64; in brackets the float32 module's own distance from float64 on the same rows.

  2a tiles, 65 716 / 65 622 listed rows, 2061 / 2053 tiles     mu max    mu mean   v max
     256 biGRU  x3                                            6.83e-06  9.48e-07  8.54e-06  (3.41e-07 4.87e-08 2.90e-07)
     256 biGRU  bf16                                          1.74e-03  3.01e-04  2.06e-03
     256 GRU    x3                                            6.39e-06  8.49e-07  6.59e-06  (3.22e-07 4.32e-08 3.41e-07)
     256 GRU    bf16                                          1.81e-03  2.92e-04  1.92e-03
     64 biGRU   x3                                            3.62e-06  6.10e-07  3.50e-06  (2.64e-07 2.77e-08 1.52e-07)
     64 biGRU   bf16                                          1.93e-03  3.39e-04  1.96e-03
     64 GRU     x3                                            4.26e-06  6.11e-07  4.72e-06  (1.90e-07 2.81e-08 2.93e-07)
     64 GRU     bf16                                          2.20e-03  3.17e-04  2.38e-03
  2b MLP, 131 269 rows
     W 39   x3   (mu before the tanh)                         1.01e-05  1.22e-06  1.15e-05  (7.53e-07 5.22e-08 5.44e-07)
     W 102  x3   (mu before the tanh)                         8.76e-06  7.51e-07  8.72e-06  (5.15e-07 3.17e-08 5.37e-07)
     W 39   bf16                                              5.96e-03  6.25e-04  5.03e-03
  2c reader, 32 795 rows: feature error against the float32 module / against float64 (the module against float64)
     256 biGRU float32                                        2.86e-06 / 2.67e-06  (2.17e-06)
     64 GRU bf16 (bound: 3e-5 + 2^-8 max|f|, one bf16 ulp)    3.11e-02 / 3.11e-02  (1.81e-06)
  2d tanh_out 0, 256 biGRU, 301 rows   x3                     3.32e-06  7.97e-07  2.48e-06  (1.81e-07 4.11e-08 1.99e-07)
                                       bf16                   1.31e-03  2.92e-04  1.05e-03
     state_dim 1 / 7 / 16, slots 1 / 5: x3 mu max 2.1e-06 .. 3.1e-06, v max 1.4e-06 .. 2.8e-06; bf16 0.9e-03 .. 1.4e-03
     non-finite rows: both come out FINITE, in both precisions, with v of an all-zero first hidden layer
  2e env scale, 401 rows
     256 biGRU  x3                                            2.24e-06  5.11e-07  2.62e-06  (1.36e-07 3.50e-08 1.41e-07)
     256 biGRU  bf16 (outside, as asserted)                   1.22e-03  2.72e-04  1.22e-03
     64 GRU     x3                                            2.35e-06  5.54e-07  2.33e-06  (1.11e-07 2.51e-08 1.76e-07)
     64 GRU     bf16 (outside, as asserted)                   1.32e-03  2.93e-04  1.37e-03

The bounds: MU_MAX 1e-4, MU_MEAN 1e-5, V_REL 1e-4 (x3); 3e-2 (bf16); 3e-5 (reader).  Every bit-for-bit comparison held.
"""
import copy
import ctypes as C
import functools

import pytest
import torch

from rvo3d_amd import _lib
from rvo3d_amd.policy import mlp_ac, rnn_ac
from test_gpu_policy_x3 import _pack, _run
from test_gpu_rnn_tiles import Space, _ac, _p, _rows, _stream
from test_gpu_rnn_tiles_x3 import Tiles, _figures, _forward64
from test_policy_trips_host import trip_sizes
from test_policy_x3_host import MU_MAX, MU_MEAN, V_REL, config3_like_obs
from test_policy_x3_host import forward64 as mlp_forward64
from test_rnn_x3_host import forward64 as pre_tanh_forward64

pytestmark = pytest.mark.gpu
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def _sizes():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return cus, trip_sizes(cus)


def _fn(precision):
    return getattr(_lib.lib(), "rvo3d_policy_rnn_tiles_x3" if precision == "x3" else "rvo3d_policy_rnn_tiles")


class Launch:
    """rvo3d_policy_rnn_tiles / _x3 with every argument in the caller's hands: max_rows and the allocation apart, the
    count word as given, outputs the caller may pass in again (sentinel 9.0), tanh_out, std_factor."""

    def __init__(self, tb, precision, max_rows, slots, alloc_rows=None):
        self.tb, self.fn, self.max_rows, self.slots = tb, _fn(precision), max_rows, slots
        self.alloc = max_rows if alloc_rows is None else alloc_rows
        nb = int(_lib.lib().rvo3d_policy_rnn_tiles_work_bytes(max_rows, slots))
        assert nb > 0
        self.work = torch.zeros(nb // 4, dtype=torch.int32, device=DEV)
        self.lst = torch.zeros(max_rows + 64, dtype=torch.int32, device=DEV)
        self.ctr = torch.zeros(2, dtype=torch.int32, device=DEV)

    def outputs(self):
        return [torch.full(s, 9.0, device=DEV) for s in ((self.alloc, 3), (self.alloc,), (self.alloc,), (self.alloc, 3))]

    def __call__(self, obs, cnt, entries, log_std, count=None, out=None, tanh=None, std_factor=1.0, seed=7, step=3):
        tb, n = self.tb, int(entries.numel())
        assert n <= self.lst.numel() and obs.shape[0] >= self.alloc and cnt.numel() >= self.alloc
        self.lst.zero_()
        self.lst[:n] = entries.to(torch.int32)
        self.ctr[0] = n if count is None else count
        out = self.outputs() if out is None else out
        tanh = tb["tanh"] if tanh is None else tanh
        _lib.check(self.fn(
            _p(tb["blob"]), tb["blob_bytes"], tb["hidden"], tb["in_dim"], tb["state_dim"], tb["bidir"], _p(obs),
            obs.stride(0), _p(cnt), _p(self.lst), _p(self.ctr), C.c_void_p(self.ctr.data_ptr() + 4), _p(self.work),
            self.max_rows, self.slots, 1 if tanh else 0, _p(log_std), std_factor, seed, step, *[_p(t) for t in out],
            _stream()), "rvo3d_policy_rnn_tiles")
        torch.cuda.synchronize()
        # count, done_blocks and the cursors are zero after every call
        assert self.ctr.tolist() == [0, 0] and int(self.work[:32].abs().sum()) == 0
        return out


def _direct_sample(mu, val, log_std, std_factor, seed, step):
    """rvo3d_policy_sample in direct mode (hidden 0) fed mu / v as they are: act, logp, val, raw."""
    rows = mu.shape[0]
    out = [torch.empty(s, device=DEV) for s in ((rows, 3), (rows,), (rows,), (rows, 3), (rows, 3))]
    hd = _lib.PolicyHeads(mu.data_ptr(), val.data_ptr(), 3, 1, _lib.RVO3D_F32, 0, 0, 0, None, None, None, None,
                          log_std.data_ptr())
    _lib.check(_lib.lib().rvo3d_policy_sample(C.byref(hd), rows, std_factor, seed, step, *[_p(t) for t in out],
                                              _stream()), "rvo3d_policy_sample")
    torch.cuda.synchronize()
    return out[0], out[1], out[2], out[4]


def _module32(ac, obs, cnt):
    with torch.no_grad():
        arg = (obs, cnt)
        d, _ = ac.pi(arg)
        return d.mean, ac.v(arg)


def _ac_sd(hidden, bi, state_dim, seed):
    """tests/test_gpu_rnn_tiles.py::_ac with another state_dim."""
    torch.manual_seed(seed)
    ac = rnn_ac(None, Space(), state_dim, 9, hidden, (256, 256), (256, 256), torch.nn.ReLU, torch.nn.Tanh,
                torch.nn.Identity, use_gpu=False, rnn_mode="biGRU" if bi else "GRU").cuda()
    with torch.no_grad():
        for p_ in ac.pi.rnn_reader.parameters():
            p_.add_(torch.randn_like(p_) * 0.2)
    return ac


def _obs_for(cnt, nm, seed, state_dim=12):
    """Rows like tests/test_gpu_rnn_tiles.py::_rows for given counts: zeros behind each row's VO rows."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    W = state_dim + 9 * nm
    obs = torch.randn((cnt.numel(), W), device=DEV, generator=g)
    obs[:, :2] *= 3.0
    obs *= (torch.arange(W, device=DEV)[None, :] < (state_dim + 9 * cnt.long().clamp(0, nm))[:, None]).float()
    return obs


# ---- 2a. tiles, several trips --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tiles_case(hidden, bi):
    """The model, the rows, the list and both references of one (hidden, bi), computed once for both precisions."""
    cus, ts = _sizes()
    nw = ts.tiles_per_trip
    nm = 12 if hidden == 256 else 3
    # rows per count: count nm fills more than nw tiles; all counts more than 2 nw; no tally a multiple of 32; more
    # listed rows than one pass of the bucket kernel takes
    per = [0] * (nm + 1)
    per[nm] = 32 * (nw + 2) + 5
    rest = 2 * nw + 2 - (nw + 3)                      # tiles the shorter counts still have to fill
    each = 32 * (-(-rest // (nm - 1))) + 7
    for c in range(1, nm):
        per[c] = each + c
    short = ts.bucket_rows_per_pass + 1 - sum(per)
    if short > 0:
        per[1] += short + 32
    per = [p + 1 if c and p % 32 == 0 else p for c, p in enumerate(per)]
    n_list = sum(per)
    rows = n_list + 3001
    g = torch.Generator(device=DEV).manual_seed(1000 + hidden + bi)
    pick = torch.randperm(rows, device=DEV, generator=g)[:n_list]       # (scattered, in random list order)
    cnt = torch.randint(0, nm + 1, (rows,), device=DEV, generator=g, dtype=torch.int32)
    by_count = torch.repeat_interleave(torch.arange(nm + 1, device=DEV), torch.tensor(per, device=DEV)).to(torch.int32)
    cnt[pick] = by_count[torch.randperm(n_list, device=DEV, generator=g)]   # (every wave of the list mixes the counts)
    obs = _obs_for(cnt, nm, 2000 + hidden + bi)
    ac = _ac(hidden, bi, 5 + hidden + bi)
    # the float64 forward and the float32 module over every listed row, once for both precisions
    sample = pick
    mu64, v64 = _forward64(ac, obs[sample], cnt[sample])
    mu32, v32 = _module32(ac, obs[sample], cnt[sample])
    return dict(ac=ac, nm=nm, rows=rows, obs=obs, cnt=cnt, pick=pick, sample=sample, mu64=mu64, v64=v64, mu32=mu32,
                v32=v32, nw=nw, bucket=ts.bucket_rows_per_pass)


@pytest.mark.parametrize("precision", ["x3", "bf16"])
@pytest.mark.parametrize("hidden,bi", [(256, True), (256, False), (64, True), (64, False)])
def test_tiles_span_several_trips(hidden, bi, precision):
    """Some waves run two longest-recurrence tiles back to back, some take three tiles, most go from a long recurrence
    to a short one; the bucket kernel makes a second pass.  Against float64 and against the same list launched in
    chunks of at most one trip: all four outputs bit for bit over the whole arrays."""
    k = _tiles_case(hidden, bi)
    ac, nm, rows, obs, cnt, pick, nw = k["ac"], k["nm"], k["rows"], k["obs"], k["cnt"], k["pick"], k["nw"]
    # the conditions the launch rests on, on THIS device
    per = torch.bincount(cnt[pick].long(), minlength=nm + 1)
    assert int(per[0]) == 0 and bool((per[1:] > 0).all()) and bool((per[1:] % 32 != 0).all())
    tiles = (per[1:] + 31) // 32
    assert int(per[nm]) > 32 * nw and int(tiles[nm - 1]) > nw           # two tiles of count nm on some waves
    assert int(tiles.sum()) > 2 * nw                                     # three tiles on some waves
    assert pick.numel() > k["bucket"]                                    # a second pass of the bucket kernel
    assert rows - pick.numel() >= 3000 and pick.unique().numel() == pick.numel()
    listed = torch.zeros(rows, dtype=torch.bool, device=DEV)
    listed[pick] = True
    assert int((listed[1:] != listed[:-1]).sum()) > 2000                 # the unlisted rows lie between the listed ones

    run = Launch(ac.rnn_tiles_blob(precision), precision, rows, nm)
    log_std = ac.log_std.detach()
    big = run(obs, cnt, pick, log_std)
    # one trip at a time into a second set of outputs
    chunk = 16 * nw
    assert chunk <= 32 * (nw - nm)
    small = run.outputs()
    for a in range(0, pick.numel(), chunk):
        run(obs, cnt, pick[a:a + chunk], log_std, out=small)
    assert -(-pick.numel() // chunk) >= 3
    for name, a, b in zip(("act", "logp", "val", "mu"), big, small):
        assert torch.equal(a, b), (name, int((a != b).sum()))
    act, logp, val, mu = big
    for t in big:
        assert bool((t[~listed] == 9.0).all()) and bool(torch.isfinite(t[pick]).all())
    s = k["sample"]
    ok, fig = _figures(mu[s], val[s], k["mu64"], k["v64"])
    _, fig32 = _figures(k["mu32"], k["v32"], k["mu64"], k["v64"])
    print(f"tiles trips hidden {hidden} bi {bi} {precision}: {pick.numel()} listed rows, {int(tiles.sum())} tiles on "
          f"{nw} waves; against float64 on {s.numel()} rows: mu max {fig[0]:.2e} mean {fig[1]:.2e}, v max {fig[2]:.2e} "
          f"(float32 module: mu max {fig32[0]:.2e} mean {fig32[1]:.2e}, v max {fig32[2]:.2e})")
    if precision == "x3":
        assert ok, fig
    else:
        assert torch.allclose(mu[s], k["mu32"], atol=3e-2, rtol=3e-2), float((mu[s] - k["mu32"]).abs().max())
        assert torch.allclose(val[s], k["v32"], atol=3e-2, rtol=3e-2), float((val[s] - k["v32"]).abs().max())


# ---- 2b. the MLP kernels, several trips ------------------------------------------------------------------------------
@pytest.mark.parametrize("W,x3", [(39, True), (102, True), (39, False)])
def test_mlp_spans_several_trips(W, x3):
    """rows = 2 trips + 3 wave chunks + 5: val and mu bit-equal to launches of at most one trip; the sample of the big
    launch (act, logp, raw) bit-equal to rvo3d_policy_sample in direct mode fed the kernel's own mu (between chunks the
    noise differs by design: its counter is the row index within the launch - so raw is compared there on the first
    chunk only, where the two indices agree)."""
    cus, ts = _sizes()
    trip = ts.mlp_rows_per_trip
    rows = 2 * trip + 64 * 3 + 5
    assert trip % 64 == 0 and rows > 2 * trip and (rows - 2 * trip) % 64 != 0
    nm = (W - 12) // 9
    g = torch.Generator(device=DEV).manual_seed(W + x3)
    torch.manual_seed(W)
    ac = mlp_ac(W).to(DEV)
    cnt = torch.randint(0, 3, (rows,), device=DEV, generator=g, dtype=torch.int32).clamp(max=nm)
    cnt[torch.rand(rows, device=DEV, generator=g) < 0.05] = nm
    cnt[trip + 64 * 7:trip + 64 * 9] = 0                   # whole empty wave chunks in the second and third trips
    cnt[2 * trip + 64:2 * trip + 128] = 0
    x = torch.randn((rows, W), device=DEV, generator=g) * 3
    x *= (torch.arange(W, device=DEV)[None, :] < (12 + 9 * cnt.long())[:, None]).float()
    log_std = torch.tensor([-1.0, -0.5, -1.5], device=DEV)
    blob = _pack(ac, W, x3=x3)
    tanh = not x3   # (x3: mu before the tanh, as its accuracy bounds are stated; bf16: the module's own mu)
    act, logp, val, mu, raw = _run(blob, W, x, log_std, tanh=tanh, seed=11, step=5, cnt=cnt, x3=x3)
    with torch.no_grad():
        z64, v64 = mlp_forward64(ac.pi_net, x), mlp_forward64(ac.v_net, x).squeeze(-1)
        z32, v32 = ac.pi_net[:-1](x).double(), ac.v_net(x).squeeze(-1).double()
    d32 = (float((z32 - z64).abs().max()), float((z32 - z64).abs().mean()), float((v32 - v64).abs().max()))
    if x3:
        d_mu, d_v = (mu.double() - z64).abs(), (val.double() - v64).abs()
        fig = (float(d_mu.max()), float(d_mu.mean()), float(d_v.max()))
        ok = fig[0] <= MU_MAX and fig[1] <= MU_MEAN and bool((d_v <= V_REL * v64.abs().clamp(min=1.0)).all())
    else:
        d_mu, d_v = (mu.double() - torch.tanh(z64)).abs(), (val.double() - v64).abs()
        fig = (float(d_mu.max()), float(d_mu.mean()), float(d_v.max()))
        ok = fig[0] < 3e-2 and fig[2] < 3e-2
    print(f"mlp trips W {W} {'x3' if x3 else 'bf16'}: {rows} rows, {trip} per trip; mu max {fig[0]:.2e} mean {fig[1]:.2e}, "
          f"v max {fig[2]:.2e} (float32 module before the tanh: mu max {d32[0]:.2e} mean {d32[1]:.2e}, v max {d32[2]:.2e})")
    assert ok, fig
    # at most one trip per launch, a multiple of 64 rows each
    parts = [_run(blob, W, x[a:a + trip], log_std, tanh=tanh, seed=11, step=5, cnt=cnt[a:a + trip], x3=x3)
             for a in range(0, rows, trip)]
    assert len(parts) == 3
    assert torch.equal(val, torch.cat([p[2] for p in parts])) and torch.equal(mu, torch.cat([p[3] for p in parts]))
    assert torch.equal(raw[:trip], parts[0][4]) and torch.equal(act[:trip], parts[0][0])
    assert torch.equal(logp[:trip], parts[0][1])
    a2, l2, v2, r2 = _direct_sample(mu, val, log_std, 1.0, 11, 5)
    assert torch.equal(act, a2) and torch.equal(logp, l2) and torch.equal(val, v2) and torch.equal(raw, r2)


# ---- 2c. the reader's first step, several trips ----------------------------------------------------------------------
@pytest.mark.parametrize("hidden,bi,dt", [(256, True, torch.float32), (64, False, torch.bfloat16)])
def test_reader_first_step_spans_several_trips(hidden, bi, dt):
    from rvo3d_amd.policy.policy_rnn_ac import rnn_Reader
    cus, ts = _sizes()
    trip = ts.reader_rows_per_trip
    rows, W = 2 * trip + 27, 39
    assert trip % 8 == 0 and rows % 8 != 0
    torch.manual_seed(hidden)
    r = rnn_Reader(12, 9, hidden, use_gpu=False, mode="biGRU" if bi else "GRU").cuda()
    with torch.no_grad():
        for p_ in r.parameters():
            p_.add_(torch.randn_like(p_) * 0.3)
    obs = torch.randn((rows, W), device=DEV)
    obs[:, 21:] = 0.0
    obs[::7, 12:21] = 0.0
    # inside the second and third trips: zero-VO runs, one row with a VO row inside an all-zero group, the ragged group
    obs[trip + 800:trip + 1600, 12:21] = 0.0
    obs[trip + 808 + 3, 12:21] = torch.randn(9, device=DEV)
    obs[2 * trip - 16:2 * trip + 16, 12:21] = 0.0          # a zero run across the boundary of trips two and three
    obs[2 * trip + 10, 15] = 0.25
    obs[2 * trip + 24:, 12:21] = 0.0                       # the ragged last group (three rows): zero, VO row, zero
    obs[2 * trip + 25, 12:21] = torch.randn(9, device=DEV)
    with torch.no_grad():
        want = r.forward_batch(obs, torch.ones(rows, dtype=torch.int64, device=DEV))
        r64 = copy.deepcopy(r).double()
        want64 = r64.forward_batch(obs.double(), torch.ones(rows, dtype=torch.int64, device=DEV))
    D = 12 + hidden
    ld = (D + 63) // 64 * 64
    gr = r.rnn_net
    f = lambda t: t.detach().float().contiguous()
    w = [f(gr.weight_ih_l0), f(gr.bias_ih_l0), f(gr.bias_hh_l0)] + \
        ([f(gr.weight_ih_l0_reverse), f(gr.bias_ih_l0_reverse), f(gr.bias_hh_l0_reverse)] if bi else [None] * 3) + \
        [f(r.ln.weight), f(r.ln.bias)]
    st = _lib.GruReader(*[None if t is None else t.data_ptr() for t in w], hidden, 9, 12, float(r.ln.eps))
    code = _lib.RVO3D_BF16 if dt == torch.bfloat16 else _lib.RVO3D_F32

    def launch(o, out):
        _lib.check(_lib.lib().rvo3d_reader_first_step(C.byref(st), _p(o), o.stride(0), o.shape[0], _p(out), code, ld,
                                                      _stream()), "rvo3d_reader_first_step")

    feat = torch.full((rows, ld), 7.0, dtype=dt, device=DEV)
    launch(obs, feat)
    parts = torch.full((rows, ld), 7.0, dtype=dt, device=DEV)
    for a in range(0, rows, trip):                          # single-trip launches, a multiple of 8 rows each
        launch(obs[a:a + trip], parts[a:a + trip])
    torch.cuda.synchronize()
    assert -(-rows // trip) == 3
    got = feat[:, :D].float()
    tol = 3e-5 if dt == torch.float32 else 3e-5 + 2 ** -8 * float(want.abs().max())
    err, err64 = float((got - want).abs().max()), float((got.double() - want64).abs().max())
    print(f"reader trips hidden {hidden} bi {bi} {dt}: {rows} rows, {trip} per trip; feature error {err:.2e} against the "
          f"float32 module, {err64:.2e} against float64 (the module itself: {float((want.double() - want64).abs().max()):.2e})")
    assert err < tol, err
    assert torch.isfinite(got).all()
    assert bool((feat[:, D:] == 7.0).all())                 # the padding columns keep their sentinel
    assert torch.equal(feat.view(torch.int16 if dt == torch.bfloat16 else torch.int32),
                       parts.view(torch.int16 if dt == torch.bfloat16 else torch.int32))


# ---- 2d. the tiles entry points' contract ----------------------------------------------------------------------------
PRECISIONS = ["x3", "bf16"]


def _within(ac, precision, mu, val, obs, cnt):
    """The accuracy bound of `precision` at these rows: x3 against float64, bf16 against the float32 module."""
    if precision == "x3":
        ok, fig = _figures(mu, val, *_forward64(ac, obs, cnt))
        return ok, fig
    mu32, v32 = _module32(ac, obs, cnt)
    return (torch.allclose(mu, mu32, atol=3e-2, rtol=3e-2) and torch.allclose(val, v32, atol=3e-2, rtol=3e-2),
            (float((mu - mu32).abs().max()), float((val - v32).abs().max())))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_tiles_skip_list_entries_outside_max_rows(precision):
    """obs, counts and outputs hold 320 rows, max_rows is 200, the list interleaves entries 200..319 with valid ones:
    the valid rows as from a clean list, rows 200..319 keep their sentinels (every entry stays inside the allocation:
    a broken filter shows up in the sentinels and cannot leave the buffers)."""
    nm, alloc, max_rows = 5, 320, 200
    ac = _ac(64, True, 61)
    obs, cnt, _ = _rows(alloc, nm, 10, 14)
    g = torch.Generator(device=DEV).manual_seed(5)
    valid = torch.randperm(max_rows, device=DEV, generator=g)[:77]
    cnt[valid] = (torch.arange(77, device=DEV, dtype=torch.int32) % nm) + 1
    cnt[max_rows:] = (torch.arange(alloc - max_rows, device=DEV, dtype=torch.int32) % nm) + 1
    obs = _obs_for(cnt, nm, 15)
    outside = torch.arange(max_rows, alloc, device=DEV)[torch.randperm(alloc - max_rows, device=DEV, generator=g)]
    mixed = torch.empty(77 + 120, dtype=torch.int64, device=DEV)
    slot = torch.zeros(197, dtype=torch.bool, device=DEV)
    slot[torch.randperm(197, device=DEV, generator=g)[:77]] = True
    mixed[slot], mixed[~slot] = valid, outside
    assert mixed.numel() <= max_rows and int((mixed >= max_rows).sum()) == 120 and int(mixed.max()) < alloc
    run = Launch(ac.rnn_tiles_blob(precision), precision, max_rows, nm, alloc_rows=alloc)
    log_std = ac.log_std.detach()
    clean = run(obs, cnt, valid, log_std)
    got = run(obs, cnt, mixed, log_std)
    for a, b in zip(clean, got):
        assert torch.equal(a, b)
        assert bool((b[max_rows:] == 9.0).all())
        assert not bool((b[valid] == 9.0).any())
    ok, fig = _within(ac, precision, got[3][valid], got[2][valid], obs[valid], cnt[valid])
    assert ok, fig


@pytest.mark.parametrize("precision", PRECISIONS)
def test_tiles_clamp_a_count_word_above_max_rows(precision):
    """count = max_rows + 50 over a full permutation: every row computed once, as from the exact count."""
    nm, rows = 5, 203
    ac = _ac(64, True, 62)
    obs, cnt, _ = _rows(rows, nm, rows, 16)
    cnt.clamp_(min=1)
    obs = _obs_for(cnt, nm, 17)
    perm = torch.randperm(rows, device=DEV)
    run = Launch(ac.rnn_tiles_blob(precision), precision, rows, nm)
    log_std = ac.log_std.detach()
    exact = run(obs, cnt, perm, log_std)
    over = run(obs, cnt, perm, log_std, count=rows + 50)
    for a, b in zip(exact, over):
        assert torch.equal(a, b) and not bool((b == 9.0).any())
    ok, fig = _within(ac, precision, over[3], over[2], obs, cnt)
    assert ok, fig


@pytest.mark.parametrize("precision", PRECISIONS)
def test_tiles_clamp_vo_count_to_the_slots(precision):
    """Listed rows with vo_count slots + 3 and 0 are computed as rows of count slots and 1."""
    nm, rows, n_list = 5, 300, 131
    ac = _ac(64, True, 63)
    obs, cnt, pick = _rows(rows, nm, n_list, 18)
    hi, lo = pick[3::10], pick[7::10]
    want_cnt = cnt.clone()
    want_cnt[hi], want_cnt[lo] = nm, 1
    obs = _obs_for(want_cnt, nm, 19)                       # (the data of the clamped counts: slots VO rows / one VO row)
    odd_cnt = want_cnt.clone()
    odd_cnt[hi], odd_cnt[lo] = nm + 3, 0
    run = Launch(ac.rnn_tiles_blob(precision), precision, rows, nm)
    log_std = ac.log_std.detach()
    want = run(obs, want_cnt, pick, log_std)
    got = run(obs, odd_cnt, pick, log_std)
    for a, b in zip(want, got):
        assert torch.equal(a, b) and not bool((b[pick] == 9.0).any())
    both = torch.cat([hi, lo])
    ok, fig = _within(ac, precision, got[3][both], got[2][both], obs[both], want_cnt[both])
    assert ok, fig


@pytest.mark.parametrize("precision", PRECISIONS)
def test_tiles_read_only_a_rows_own_columns(precision):
    """obs as a view of a wider buffer (obs_ld = W + 7) whose padding is NaN, every column behind a row's own vo_count VO
    rows NaN as well: bit-equal to the contiguous, zero-filled rows, and finite."""
    nm, rows, n_list = 5, 300, 131
    W = 12 + 9 * nm
    ac = _ac(64, True, 64)
    obs, cnt, pick = _rows(rows, nm, n_list, 20)
    wide = torch.full((rows, W + 7), float("nan"), device=DEV)
    view = wide[:, :W]
    view.copy_(obs)
    behind = torch.arange(W, device=DEV)[None, :] >= (12 + 9 * cnt.long().clamp(1, nm))[:, None]
    view[behind] = float("nan")
    assert view.stride(0) == W + 7 and view.data_ptr() == wide.data_ptr() and bool(torch.isnan(view[pick]).any())
    run = Launch(ac.rnn_tiles_blob(precision), precision, rows, nm)
    log_std = ac.log_std.detach()
    want = run(obs, cnt, pick, log_std)
    got = run(view, cnt, pick, log_std)
    for a, b in zip(want, got):
        assert torch.equal(a, b) and bool(torch.isfinite(b[pick]).all())


@pytest.mark.parametrize("precision", PRECISIONS)
def test_tiles_without_tanh_and_with_other_std_factors(precision):
    """tanh_out = 0: dbg_mu is the stack's output itself (x3: within MU_MAX / MU_MEAN / V_REL of the float64 forward
    before the tanh; bf16: within 3e-2 of the float32 module's); std_factor 0.5 and 0.0 (std clamps at 1e-4): act and
    logp bit-equal to rvo3d_policy_sample in direct mode with the same std_factor, fed the kernel's mu."""
    nm, rows, n_list = 10, 700, 301
    ac = _ac(256, True, 65)
    obs, cnt, pick = _rows(rows, nm, n_list, 21)
    run = Launch(ac.rnn_tiles_blob(precision), precision, rows, nm)
    log_std = ac.log_std.detach()
    with torch.no_grad():
        z64, v64 = pre_tanh_forward64(ac, obs[pick], cnt[pick].long())
        f32 = ac.pi.rnn_reader.forward_batch(obs[pick], cnt[pick].long())
        z32, v32 = ac.pi.net_out[:-1](f32), ac.v.v_net(f32).squeeze(-1)
    assert float((torch.tanh(z64) - z64).abs().max()) > 1e-3   # (a tanh applied all the same would show)
    for sf in (0.5, 0.0):
        act, logp, val, mu = run(obs, cnt, pick, log_std, tanh=False, std_factor=sf, seed=12345, step=77)
        ok, fig = _figures(mu[pick], val[pick], z64, v64)
        _, fig32 = _figures(z32, v32, z64, v64)
        print(f"tiles tanh_out 0 std_factor {sf} {precision}: mu max {fig[0]:.2e} mean {fig[1]:.2e}, v max {fig[2]:.2e} "
              f"(float32 module: mu max {fig32[0]:.2e} mean {fig32[1]:.2e}, v max {fig32[2]:.2e})")
        if precision == "x3":
            assert ok, fig
        else:
            assert torch.allclose(mu[pick], z32, atol=3e-2, rtol=3e-2) and torch.allclose(val[pick], v32, atol=3e-2, rtol=3e-2)
        a2, l2, v2, _ = _direct_sample(mu, val, log_std, sf, 12345, 77)
        assert torch.equal(act[pick], a2[pick]) and torch.equal(logp[pick], l2[pick]) and torch.equal(val[pick], v2[pick])
        std = min(max(sf * float(torch.exp(log_std[0])) + 1e-6, 1e-4), 10.0)
        assert float((act[pick] - mu[pick]).abs().max()) <= 6 * std + 5.1e-3    # (rounded to 0.01; six sigma)


@pytest.mark.parametrize("state_dim", [1, 7, 16])
@pytest.mark.parametrize("hidden,bi", [(64, False), (256, True)])
def test_tiles_other_state_dims_and_slots(hidden, bi, state_dim):
    """state_dim 1, 7, 16 (the documented range's ends and an odd one) with slots 1 and 5: mu and v against the float64
    forward (x3) / the float32 module (bf16)."""
    ac = _ac_sd(hidden, bi, state_dim, 70 + state_dim)
    log_std = ac.log_std.detach()
    for slots in (1, 5):
        rows, n_list = 260, 101
        g = torch.Generator(device=DEV).manual_seed(slots)
        pick = torch.randperm(rows, device=DEV, generator=g)[:n_list]
        cnt = torch.randint(0, slots + 1, (rows,), device=DEV, generator=g, dtype=torch.int32)
        cnt[pick] = (torch.arange(n_list, device=DEV, dtype=torch.int32) % slots) + 1
        obs = _obs_for(cnt, slots, 80 + slots, state_dim=state_dim)
        assert obs.shape[1] == state_dim + 9 * slots
        for precision in PRECISIONS:
            tb = ac.rnn_tiles_blob(precision)
            assert tb is not None and tb["state_dim"] == state_dim
            out = Launch(tb, precision, rows, slots)(obs, cnt, pick, log_std)
            ok, fig = _within(ac, precision, out[3][pick], out[2][pick], obs[pick], cnt[pick])
            print(f"tiles state_dim {state_dim} slots {slots} hidden {hidden} bi {bi} {precision}: {fig}")
            assert ok, (slots, precision, fig)
            untouched = torch.ones(rows, dtype=torch.bool, device=DEV)
            untouched[pick] = False
            assert all(bool((t[untouched] == 9.0).all()) and bool(torch.isfinite(t[pick]).all()) for t in out)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_tiles_non_finite_rows_leave_their_tile_mates_alone(precision):
    """One full 32-row tile of count 4 with a NaN in a VO row of one row and +inf in a proprio column of another: the
    other 30 rows as in a run where the two hold finite data; the two rows themselves are written (their values are
    printed, not asserted: non-finite observations are the env's error flag's business)."""
    nm, rows = 5, 200
    ac = _ac(64, True, 66)
    g = torch.Generator(device=DEV).manual_seed(9)
    pick = torch.randperm(rows, device=DEV, generator=g)[:32 + 45]
    cnt = torch.randint(0, nm + 1, (rows,), device=DEV, generator=g, dtype=torch.int32)
    cnt[pick[:32]] = 4                                      # exactly one tile of count 4 ...
    cnt[pick[32:]] = torch.tensor([1, 2, 3, 5], device=DEV, dtype=torch.int32).repeat(12)[:45]   # ... beside other counts
    obs = _obs_for(cnt, nm, 22)
    bad_nan, bad_inf = int(pick[5]), int(pick[20])
    dirty = obs.clone()
    dirty[bad_nan, 12 + 9 * 2 + 4] = float("nan")
    dirty[bad_inf, 3] = float("inf")
    run = Launch(ac.rnn_tiles_blob(precision), precision, rows, nm)
    log_std = ac.log_std.detach()
    want = run(obs, cnt, pick, log_std)
    got = run(dirty, cnt, pick, log_std)
    mates = torch.ones(rows, dtype=torch.bool, device=DEV)
    mates[bad_nan] = mates[bad_inf] = False
    for a, b in zip(want, got):
        assert torch.equal(a[mates], b[mates])
        for row in (bad_nan, bad_inf):
            assert not bool((b[row] == 9.0).any()), row      # written, whatever it holds
    print(f"non-finite rows {precision}: NaN in a VO row -> act {got[0][bad_nan].tolist()} logp {float(got[1][bad_nan])} "
          f"val {float(got[2][bad_nan])}; +inf in the state -> act {got[0][bad_inf].tolist()} "
          f"logp {float(got[1][bad_inf])} val {float(got[2][bad_inf])}")


# ---- 2e. accuracy at the env's scale ---------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden,bi", [(256, True), (64, False)])
def test_tiles_accuracy_at_env_scale(hidden, bi):
    """config-3-like rows (positions up to 50, every row with VO rows): the x3 kernel inside MU_MAX / MU_MEAN / V_REL of
    the float64 forward, the bf16 kernel outside (tests/test_policy_trips_host.py: the emulation on the same rows)."""
    nm, rows, n_list = 12, 1001, 401
    ac = _ac(hidden, bi, 5 + hidden + bi)
    obs, cnt = config3_like_obs(rows, 12 + 9 * nm, vo_share=1.0, seed=3)
    obs, cnt = obs.to(DEV), cnt.to(DEV).to(torch.int32)
    pick = torch.randperm(rows, device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))[:n_list]
    assert int(cnt.min()) >= 1 and float(obs[pick][:, :12].abs().max()) > 40.0
    mu64, v64 = _forward64(ac, obs[pick], cnt[pick])
    _, fig32 = _figures(*_module32(ac, obs[pick], cnt[pick]), mu64, v64)
    for precision in PRECISIONS:
        run = Tiles(ac, rows, nm, precision)
        act, logp, val, mu = run(obs, cnt, pick)
        assert run.clean()
        ok, fig = _figures(mu[pick], val[pick], mu64, v64)
        print(f"env scale hidden {hidden} bi {bi} {precision}: mu max {fig[0]:.2e} mean {fig[1]:.2e}, v max {fig[2]:.2e} "
              f"(float32 module: mu max {fig32[0]:.2e} mean {fig32[1]:.2e}, v max {fig32[2]:.2e})")
        assert bool(torch.isfinite(mu[pick]).all())
        if precision == "x3":
            assert ok, fig
        else:
            assert not ok, fig
