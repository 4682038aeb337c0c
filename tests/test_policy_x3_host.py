"""The float32-class policy step (rvo3d_policy_mlp_x3_sample) on the host side: the trainer's keyword, the C-ABI's
symbol list, and the error model the GPU bounds of tests/test_gpu_policy_x3.py rest on - a PyTorch emulation of the
split-bf16 products (a_hi b_hi + a_lo b_hi + a_hi b_lo, hi = bf16_rne(x), lo = bf16_rne(x - hi)) against a float64
forward of the default-initialised MLP(256, 256) on config-3-like observations, next to plain bf16 operands."""
import pytest
import torch

from rvo3d_amd import _lib
from rvo3d_amd.policy import mlp_ac, multi_ppo

# the GPU bounds (tests/test_gpu_policy_x3.py, check 2): mu before the tanh and v against the float64 forward
MU_MAX, MU_MEAN, V_REL = 1e-4, 1e-5, 1e-4


def split(t):
    """float32 tensor -> (hi, lo) as float64: hi = bf16_rne(t), lo = bf16_rne(t - hi)."""
    t = t.float()
    hi = t.to(torch.bfloat16).float()
    lo = (t - hi).to(torch.bfloat16).float()
    return hi.double(), lo.double()


def x3_linear(x, w, b_split=None, b_f32=None):
    """x [rows][k] float32 activations, w [out][k] float32: the three products of the kernel (float64 sums stand in
    for its float32 accumulation); the first layer's bias split like a weight column, the others added in float32."""
    xh, xl = split(x)
    wh, wl = split(w)
    y = xh @ wh.T + xh @ wl.T + xl @ wh.T
    if b_split is not None:
        bh, bl = split(b_split)
        y = y + bh + bl
    if b_f32 is not None:
        y = y + b_f32.double()
    return y.float()


def emulate_x3(net, x):
    """The kernel's arithmetic on one mlp() stack: float32 pre-activation of the last layer (before Tanh)."""
    lin = [m for m in net if isinstance(m, torch.nn.Linear)]
    h = torch.relu(x3_linear(x, lin[0].weight, b_split=lin[0].bias))
    h = torch.relu(x3_linear(h, lin[1].weight, b_f32=lin[1].bias))
    return x3_linear(h, lin[2].weight, b_f32=lin[2].bias)


def emulate_bf16(net, x):
    """The bf16 kernel's arithmetic (tests/test_gpu_rollout.py's emulation): bf16 operands, float32 sums."""
    bf = torch.bfloat16
    lin = [m for m in net if isinstance(m, torch.nn.Linear)]
    h = x.to(bf).double()
    h = torch.relu(h @ lin[0].weight.to(bf).double().T + lin[0].bias.to(bf).double()).float().to(bf).double()
    h = torch.relu(h @ lin[1].weight.to(bf).double().T + lin[1].bias.double()).float().to(bf).double()
    return (h @ lin[2].weight.to(bf).double().T + lin[2].bias.double()).float()


def forward64(net, x):
    lin = [m for m in net if isinstance(m, torch.nn.Linear)]
    h = x.double()
    for i, m in enumerate(lin):
        h = h @ m.weight.double().T + m.bias.double()
        if i < len(lin) - 1:
            h = torch.relu(h)
    return h


def config3_like_obs(rows, width, vo_share=0.1, seed=0):
    """Rows shaped like the env's: 12 state floats (positions up to 50), 9 per kept velocity-obstacle row, zeros behind;
    `vo_share` of the rows carry 1..nm VO rows."""
    g = torch.Generator().manual_seed(seed)
    nm = (width - 12) // 9
    x = torch.zeros((rows, width))
    x[:, 0:3] = torch.rand((rows, 3), generator=g) * 50          # position
    x[:, 3:6] = torch.randn((rows, 3), generator=g)              # velocity
    x[:, 6:9] = torch.rand((rows, 3), generator=g) * 50          # goal / waypoint
    x[:, 9:12] = torch.rand((rows, 3), generator=g) * 6.3 - 3.1  # angles, distance terms
    cnt = torch.zeros(rows, dtype=torch.int32)
    has = torch.rand(rows, generator=g) < vo_share
    cnt[has] = torch.randint(1, nm + 1, (int(has.sum()),), generator=g, dtype=torch.int32)
    vo = torch.randn((rows, 9 * nm), generator=g) * 3
    vo[:, 0::9] = torch.rand((rows, nm), generator=g) * 50       # an obstacle's position terms
    keep = torch.arange(9 * nm)[None, :] < 9 * cnt[:, None]
    x[:, 12:12 + 9 * nm] = vo * keep
    return x, cnt


def test_fused_mlp_fp32_with_amp_is_rejected():
    """fused_mlp_fp32 selects the float32 rollout's kernel; with amp=True the keyword is a contradiction."""
    ac = mlp_ac(102)
    with pytest.raises(ValueError, match="fused_mlp_fp32"):
        multi_ppo(object(), ac, amp=True, fused_mlp_fp32=True)


def test_symbols_list_the_x3_entry_points():
    for s in ("rvo3d_policy_mlp_x3_blob_bytes", "rvo3d_policy_mlp_x3_pack", "rvo3d_policy_mlp_x3_sample"):
        assert s in _lib.SYMBOLS


def test_mlp_blob_rejects_an_unknown_precision():
    with pytest.raises(ValueError, match="precision"):
        mlp_ac(102).mlp_blob("fp16")


@pytest.mark.parametrize("width", [102, 57, 39, 120])
def test_split_bf16_error_model(width):
    """The emulated split-bf16 forward stays inside the GPU bounds against float64; bf16 operands exceed them by far."""
    torch.manual_seed(width)
    ac = mlp_ac(width)
    x, cnt = config3_like_obs(4096, width, seed=width)
    assert float((cnt > 0).float().mean()) >= 0.08
    with torch.no_grad():
        z64, v64 = forward64(ac.pi_net, x), forward64(ac.v_net, x).squeeze(-1)
        z3, v3 = emulate_x3(ac.pi_net, x).double(), emulate_x3(ac.v_net, x).squeeze(-1).double()
        zb, vb = emulate_bf16(ac.pi_net, x).double(), emulate_bf16(ac.v_net, x).squeeze(-1).double()
    d_mu, d_v = (z3 - z64).abs(), (v3 - v64).abs()
    assert float(d_mu.max()) <= MU_MAX and float(d_mu.mean()) <= MU_MEAN, (float(d_mu.max()), float(d_mu.mean()))
    assert bool((d_v <= V_REL * v64.abs().clamp(min=1.0)).all()), float(d_v.max())
    # plain bf16 operands: far outside
    assert float((zb - z64).abs().max()) > 1e-3 and float((vb - v64).abs().max()) > 1e-3
    # (the float32 module itself sits well inside)
    with torch.no_grad():
        z32 = ac.pi_net[:-1](x).double()
    assert float((z32 - z64).abs().max()) < 1e-5


@pytest.mark.parametrize("name", ["rvo3d_policy_mlp", "rvo3d_policy_mlp_x3"])
def test_mlp_entry_points_reject_bad_arguments_before_any_launch(name):
    """The argument checks of the bf16 and x3 entry points (one implementation in csrc/rvo3d_capi.hip) on the CPU: fake
    aligned pointers, never dereferenced - every call below fails its checks, or has no rows, before touching a GPU."""
    import ctypes as C
    _lib.build_hip()
    L = _lib.lib()
    fake = lambda n: C.c_void_p(4096 * n)
    sample, pack, nbytes = (getattr(L, name + s) for s in ("_sample", "_pack", "_blob_bytes"))
    W, rows = 102, 200
    args = lambda **k: [k.get("blob", fake(1)), k.get("W", W), fake(2), k.get("ld", W), k.get("rows", rows), None, 12, 9,
                        1, fake(3), 1.0, 0, 0, fake(4), fake(5), fake(6), None, None, None]
    assert sample(*args(W=127)) == -1 and b"obs_width" in L.rvo3d_last_error()
    assert sample(*args(ld=W - 1)) == -1 and b"obs_ld" in L.rvo3d_last_error()
    assert sample(*args(blob=C.c_void_p(4096 + 4))) == -1 and b"aligned" in L.rvo3d_last_error()
    assert sample(*args(rows=-1)) == -1 and b"rows" in L.rvo3d_last_error()
    assert sample(*args(blob=None)) == -1 and b"null" in L.rvo3d_last_error()
    assert sample(*args(rows=0)) == 0
    assert nbytes(127) == -1 and nbytes(0) == -1
    assert nbytes(102) == {"rvo3d_policy_mlp": 2 * (7 * 8192 + 131072 + 1024 + 2048 + 16),
                           "rvo3d_policy_mlp_x3": 2 * (7 * 16384 + 131072 + 1024 + 4096 + 131072 + 16)}[name]
    w = _lib.MlpWeights(*[fake(10 + i) for i in range(6)])
    assert pack(None, C.byref(w), W, fake(1), None) == -1 and b"null" in L.rvo3d_last_error()
    assert pack(C.byref(w), C.byref(w), 127, fake(1), None) == -1 and b"obs_width" in L.rvo3d_last_error()
    assert pack(C.byref(w), C.byref(w), W, C.c_void_p(4096 + 8), None) == -1 and b"aligned" in L.rvo3d_last_error()
    bad = _lib.MlpWeights.from_buffer_copy(w)
    bad.w2 = None
    assert pack(C.byref(w), C.byref(bad), W, fake(1), None) == -1 and b"weight" in L.rvo3d_last_error()
