"""The float32-class biGRU policy step (rvo3d_policy_rnn_tiles_x3, zero_vo_plan("x3"), multi_ppo(fused_rnn_fp32=True)) on
the host side: the error model the GPU bounds of tests/test_gpu_rnn_tiles_x3.py rest on - a PyTorch emulation of the
kernels' split-bf16 products (a_hi b_hi + a_hi b_lo + a_lo b_hi, float64 sums standing in for the float32 accumulation)
against a float64 forward of the modules, next to bf16 stacks -, the new C-ABI symbols, their size queries and argument
checks (fake pointers: every call fails before anything touches a GPU), and the new keywords' refusals."""
import copy
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT
from rvo3d_amd import _lib
from rvo3d_amd.policy import multi_ppo, rnn_ac
from rvo3d_amd.policy.policy_rnn_ac import _zero_input_h0, collapsed_first_layer
from test_policy_x3_host import MU_MAX, MU_MEAN, V_REL, config3_like_obs, split

NEW = ("rvo3d_policy_rnn_tiles_x3_blob_bytes", "rvo3d_policy_rnn_tiles_x3_pack", "rvo3d_policy_rnn_tiles_x3")


class Space:
    shape = (3,)


def _ac(hidden, bi, seed):
    """tests/test_gpu_rnn_tiles.py::_ac on the CPU: (256, 256) heads, the reader's parameters perturbed by 0.2."""
    torch.manual_seed(seed)
    ac = rnn_ac(None, Space(), 12, 9, hidden, (256, 256), (256, 256), torch.nn.ReLU, torch.nn.Tanh, torch.nn.Identity,
                use_gpu=False, rnn_mode="biGRU" if bi else "GRU")
    with torch.no_grad():
        for p_ in ac.pi.rnn_reader.parameters():
            p_.add_(torch.randn_like(p_) * 0.2)
    return ac


def _rows(rows, nm, seed):
    """obs [rows, 12 + 9 nm] with counts 1..nm in turn, zeros behind each row's VO rows."""
    g = torch.Generator().manual_seed(seed)
    W = 12 + 9 * nm
    cnt = (torch.arange(rows) % nm) + 1
    obs = torch.randn((rows, W), generator=g)
    obs[:, :12] *= torch.tensor([3., 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1])
    obs *= (torch.arange(W)[None, :] < (12 + 9 * cnt)[:, None]).float()
    return obs, cnt


# ---- the products: float64 results of float32 operands -------------------------------------------------------------
def mm_exact(x, w):
    return x.double() @ w.double().T


def mm_x3(x, w):
    xh, xl = split(x)
    wh, wl = split(w)
    return xh @ wh.T + xh @ wl.T + xl @ wh.T


def mm_bf16(x, w):
    bf = torch.bfloat16
    return x.to(bf).double() @ w.to(bf).double().T


def _gru_dir(g, sfx, x, lens, reverse, mm):
    """One direction as policy_rnn_tiles_kernel runs it: the biases initialise the float32 sums (b_i + b_h for r and z,
    b_in / b_hn for n), the products come on top, gate math and the state in float32; masked like rnn_Reader._gru_dir."""
    w_ih, w_hh = getattr(g, "weight_ih_l0" + sfx), getattr(g, "weight_hh_l0" + sfx)
    b_ih, b_hh = getattr(g, "bias_ih_l0" + sfx), getattr(g, "bias_hh_l0" + sfx)
    B, S, _ = x.shape
    H = w_hh.shape[1]
    h = torch.zeros((B, H))
    for t in (range(S - 1, -1, -1) if reverse else range(S)):
        gi, gh = mm(x[:, t], w_ih), mm(h, w_hh)
        brz = (b_ih + b_hh)[:2 * H].double()
        rz = torch.sigmoid((brz + gi[:, :2 * H] + gh[:, :2 * H]).float())
        rg, zg = rz[:, :H], rz[:, H:]
        i_n = (b_ih[2 * H:].double() + gi[:, 2 * H:]).float()
        h_n = (b_hh[2 * H:].double() + gh[:, 2 * H:]).float()
        hn = (1 - zg) * torch.tanh(i_n + rg * h_n) + zg * h
        h = torch.where((lens > t).unsqueeze(1), hn, h)
    return h


def _stack(net, f, mm):
    """relu(W1 f + b1) -> relu(W2 . + b2) -> W3 . + b3 before the output activation: biases in float32 on the float32
    sums, the activations float32 (the operands' rounding is mm's)."""
    lin = [m for m in net if isinstance(m, torch.nn.Linear)]
    h = f
    for i, m in enumerate(lin):
        h = (mm(h, m.weight) + m.bias.double()).float()
        if i < len(lin) - 1:
            h = torch.relu(h)
    return h


def emulate_rows(ac, obs, lens, mm_gru, mm_stack):
    """(mu before the tanh, v) float32 of rows WITH VO rows: reader with mm_gru's products, stacks with mm_stack's."""
    r = ac.pi.rnn_reader
    B = obs.shape[0]
    S = (obs.shape[1] - 12) // 9
    x = obs[:, 12:].reshape(B, S, 9)
    h = _gru_dir(r.rnn_net, "", x, lens, False, mm_gru)
    if r.mode == "biGRU":
        h = h + _gru_dir(r.rnn_net, "_reverse", x, lens, True, mm_gru)
    f = r.ln(torch.cat((obs[:, :12], h), 1))
    return _stack(ac.pi.net_out, f, mm_stack), _stack(ac.v.v_net, f, mm_stack).squeeze(-1)


def forward64(ac, obs, lens):
    a64 = copy.deepcopy(ac).double()
    f = a64.pi.rnn_reader.forward_batch(obs.double(), lens)
    return a64.pi.net_out[:-1](f), a64.v.v_net(f).squeeze(-1)


def emulate_zero_vo(ac, obs, x3):
    """(mu before the tanh, v) of rows WITHOUT a VO row as rvo3d_reader_zero_features + the MLP kernel on
    zero_vo_plan(precision) compute them: the collapsed first layer over state_dim + 8 inputs."""
    r = ac.pi.rnn_reader
    sd, D = r.state_dim, r.state_dim + r.hidden_dim
    h0 = _zero_input_h0(r, torch.device("cpu"))
    head = lambda t: t.float().to(torch.bfloat16).float()
    p = obs[:, :sd]
    t1 = p.sum(1) + float(h0.sum())
    t2 = (p * p).sum(1) + float((h0 * h0).sum())
    mean = t1 / D
    rstd = 1.0 / torch.sqrt(torch.clamp(t2 / D - mean * mean, min=0.0) + r.ln.eps)
    m = mean * rstd
    one = torch.ones_like(m)
    X = torch.cat([(p - mean[:, None]) * rstd[:, None] * r.ln.weight[:sd] + r.ln.bias[:sd],
                   torch.stack([head(rstd), head(rstd), rstd - head(rstd), head(m), head(m), m - head(m), one, one], 1)], 1)
    out = []
    for net in (ac.pi.net_out, ac.v.v_net):
        lin = [q for q in net if isinstance(q, torch.nn.Linear)]
        Wp, a, b, c = collapsed_first_layer(r, lin[0], h0)
        cols = [Wp.float()]
        for vec in (a, -b):
            v = vec.float()
            cols += [v[:, None], torch.zeros_like(v)[:, None], v[:, None]] if x3 else \
                [head(v)[:, None], (v - head(v))[:, None], head(v)[:, None]]
        cf = c.float()
        cols += [cf[:, None], (c - cf.double()).float()[:, None]] if x3 else [head(cf)[:, None], (cf - head(cf))[:, None]]
        W1 = torch.cat(cols, 1)
        mm = mm_x3 if x3 else mm_bf16
        h = torch.relu(mm(X, W1).float())
        h = torch.relu((mm(h, lin[1].weight) + lin[1].bias.double()).float())
        out.append((mm(h, lin[2].weight) + lin[2].bias.double()).float())
    return out[0], out[1].squeeze(-1)


def _inside(z, v, z64, v64):
    d_mu, d_v = (z.double() - z64).abs(), (v.double() - v64).abs()
    return (float(d_mu.max()) <= MU_MAX and float(d_mu.mean()) <= MU_MEAN
            and bool((d_v <= V_REL * v64.abs().clamp(min=1.0)).all())), (float(d_mu.max()), float(d_mu.mean()), float(d_v.max()))


@pytest.mark.parametrize("hidden,bi", [(256, True), (256, False), (64, True), (64, False)])
def test_split_bf16_error_model_of_the_rnn_paths(hidden, bi):
    """Every product split: inside MU_MAX / MU_MEAN / V_REL against float64 on the rows with VO rows (counts 1..12) and
    on the zero-VO rows (collapsed layer); the split GRU with bf16 stacks (today's "rnn_tiles") and the bf16 collapsed
    layer fall outside.  The emulation with exact products is the module's float32 forward."""
    ac = _ac(hidden, bi, 5 + hidden + bi)
    obs, cnt = _rows(1024, 12, 11)
    with torch.no_grad():
        z64, v64 = forward64(ac, obs, cnt)
        # the emulation itself: exact products give the module's own float32 forward
        ze, ve = emulate_rows(ac, obs, cnt, mm_exact, mm_exact)
        f32 = ac.pi.rnn_reader.forward_batch(obs, cnt)
        zm, vm = ac.pi.net_out[:-1](f32), ac.v.v_net(f32).squeeze(-1)
        assert float((ze - zm).abs().max()) < 1e-5 and float((ve - vm).abs().max()) < 1e-5
        assert float((zm.double() - z64).abs().max()) < 1e-5
        ok, fig = _inside(*emulate_rows(ac, obs, cnt, mm_x3, mm_x3), z64, v64)
        assert ok, fig
        ok, fig = _inside(*emulate_rows(ac, obs, cnt, mm_x3, mm_bf16), z64, v64)
        assert not ok and fig[0] > MU_MAX and fig[1] > MU_MEAN, fig
        # zero-VO rows
        x0, _ = config3_like_obs(4096, 12 + 9 * 10, vo_share=0.0, seed=hidden + bi)
        l0 = torch.ones(4096, dtype=torch.int64)
        z64, v64 = forward64(ac, x0, l0)
        ok, fig = _inside(*emulate_zero_vo(ac, x0, True), z64, v64)
        assert ok, fig
        ok, fig = _inside(*emulate_zero_vo(ac, x0, False), z64, v64)
        assert not ok and fig[0] > MU_MAX and fig[1] > MU_MEAN, fig


# ---- C-ABI and arguments ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    _lib.build_hip()
    return _lib.lib()


def test_x3_symbols_declared_listed_and_exported(L):
    hdr = open(os.path.join(ROOT, "include", "rvo3d.h")).read()
    declared = set(re.findall(r"\b(rvo3d_[a-z_0-9]+)\s*\(", hdr))
    for s in NEW:
        assert s in declared and s in _lib.SYMBOLS and hasattr(L, s)


def test_x3_size_queries(L):
    b3, b = L.rvo3d_policy_rnn_tiles_x3_blob_bytes, L.rvo3d_policy_rnn_tiles_blob_bytes
    for h in (64, 256):
        for bi in (0, 1):
            n3, n = b3(h, 9, 12, bi), b(h, 9, 12, bi)
            assert n3 > 0 and n3 % 16 == 0 and n3 > n
            # the stacks' fragments twice: 2 x (8 (h / 16 + 1) + 8 x 16 + 16) KB more
            assert n3 - n == 2 * (8 * (h // 16 + 1) + 128 + 16) * 1024
    for bad in ((128, 9, 12, 1), (0, 9, 12, 1), (256, 8, 12, 1), (256, 9, 0, 1), (256, 9, 17, 0)):
        assert b(*bad) == -1 and b3(*bad) == -1


def _fake(n):
    return C.c_void_p(4096 * n)   # (never dereferenced: every call below fails its argument checks first)


def test_x3_bad_arguments_fail_before_any_launch(L):
    """tests/test_rnn_tiles_host.py's matrix against the x3 triple; and a bf16-sized blob given to the x3 call."""
    nb = L.rvo3d_policy_rnn_tiles_x3_blob_bytes(256, 9, 12, 1)

    def call(**kw):
        a = dict(blob=_fake(1), blob_bytes=nb, hidden=256, in_dim=9, state_dim=12, bidir=1, obs=_fake(2), obs_ld=102,
                 cnt=_fake(3), lst=_fake(4), count=_fake(5), done=_fake(6), work=_fake(7), max_rows=1000, slots=10,
                 tanh=1, log_std=_fake(8), std=1.0, seed=7, step=0, act=_fake(9), logp=_fake(10), val=_fake(11),
                 mu=None, stream=None)
        a.update(kw)
        return L.rvo3d_policy_rnn_tiles_x3(*a.values())

    for kw in (dict(hidden=128), dict(hidden=64), dict(in_dim=8), dict(state_dim=17), dict(slots=0), dict(slots=13),
               dict(bidir=0), dict(blob_bytes=nb - 16), dict(obs=None), dict(cnt=None), dict(lst=None),
               dict(count=None), dict(done=None), dict(work=None), dict(act=None), dict(logp=None), dict(val=None),
               dict(log_std=None), dict(blob=None), dict(obs_ld=101), dict(max_rows=0), dict(blob=C.c_void_p(4096 + 8))):
        assert call(**kw) == -1, kw
        assert L.rvo3d_last_error()
    assert call(hidden=64) == -1 and b"another" in L.rvo3d_last_error()
    # the other precision's blob (its size says so): refused by either call
    assert call(blob_bytes=L.rvo3d_policy_rnn_tiles_blob_bytes(256, 9, 12, 1)) == -1 and b"another" in L.rvo3d_last_error()
    w = [_fake(20 + i) for i in range(10)]
    net = _lib.RnnPolicy(*w, 256, 9, 12, 0, 1e-5, 0, _lib.MlpWeights(*[_fake(40 + i) for i in range(6)]),
                         _lib.MlpWeights(*[_fake(50 + i) for i in range(6)]))
    pk = L.rvo3d_policy_rnn_tiles_x3_pack
    assert pk(None, _fake(1), nb, None) == -1
    assert pk(C.byref(net), None, nb, None) == -1
    assert pk(C.byref(net), _fake(1), nb - 16, None) == -1
    assert pk(C.byref(net), _fake(1), L.rvo3d_policy_rnn_tiles_x3_blob_bytes(256, 9, 12, 0), None) == -1  # packed for GRU
    assert pk(C.byref(net), _fake(1), L.rvo3d_policy_rnn_tiles_blob_bytes(256, 9, 12, 1), None) == -1     # the bf16 size
    for field, v in (("hidden", 100), ("in_dim", 10), ("state_dim", 20)):
        bad = _lib.RnnPolicy.from_buffer_copy(net)
        setattr(bad, field, v)
        assert pk(C.byref(bad), _fake(1), nb, None) == -1
    bad = _lib.RnnPolicy.from_buffer_copy(net)
    bad.w_hh_r = None                                                     # half a reverse direction
    assert pk(C.byref(bad), _fake(1), nb, None) == -1
    bad = _lib.RnnPolicy.from_buffer_copy(net)
    bad.pi.w2 = None
    assert pk(C.byref(bad), _fake(1), nb, None) == -1


def test_fused_rnn_fp32_with_amp_is_rejected():
    """fused_rnn_fp32 selects the float32 rollout's kernels; with amp=True the keyword is a contradiction."""
    with pytest.raises(ValueError, match="fused_rnn_fp32"):
        multi_ppo(object(), _ac(64, True, 0), amp=True, fused_rnn_fp32=True)


def test_rnn_plans_reject_an_unknown_precision():
    ac = _ac(64, True, 0)
    with pytest.raises(ValueError, match="precision"):
        ac.rnn_tiles_blob("fp16")
    with pytest.raises(ValueError, match="precision"):
        ac.zero_vo_plan("fp16")
    assert ac.rnn_tiles_blob() is None and ac.zero_vo_plan() is None     # (on the CPU: what they were)
