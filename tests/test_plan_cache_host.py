"""Host logic of the rollout's plan caches (policy_rnn_ac._plan_cached, _cast_cached), no GPU: everything the fast
paths launch is packed from the parameters ahead of time and keyed by (tag, parameter versions, parameter storages).
A training run is collect -> update -> collect, so a key that misses a kind of parameter change means rollouts on the
previous weights.  The cases: every way a parameter's value can change between two rollouts rebuilds exactly once; what
leaves the values alone (forward / backward, zero_grad, reading) rebuilds nothing."""
import gc

import pytest
import torch

from rvo3d_amd.policy import KernelPolicyStep, mlp_ac, rnn_ac
from rvo3d_amd.policy import policy_rnn_ac as P


class Space:
    shape = (3,)


def _mlp(seed=0):
    torch.manual_seed(seed)
    return mlp_ac(30)


def _rnn(seed=0, mode="biGRU"):
    torch.manual_seed(seed)
    return rnn_ac(None, Space(), 12, 9, 256, (256, 256), (256, 256), torch.nn.ReLU, torch.nn.Tanh, torch.nn.Identity,
                  use_gpu=False, rnn_mode=mode)


class Counter:
    """A `build` that counts its calls and records what it was handed as the previous value."""

    def __init__(self):
        self.calls, self.prev = 0, []

    def __call__(self, prev):
        self.calls += 1
        self.prev.append(prev)
        return {"n": self.calls}


def _get(ac, build, tag=None):
    return P._plan_cached(ac, "_test_plan", list(ac.parameters()), build, tag=tag)


def _loss(ac):
    x = torch.randn(8, 30)
    d, _ = ac.pi(x)
    return (d.mean ** 2).sum() + (ac.v(x) ** 2).sum()


def _optimizer_step(ac):
    opt = torch.optim.Adam(ac.parameters(), lr=1e-3)
    _loss(ac).backward()
    opt.step()


def _load_other(ac):
    ac.load_state_dict(_mlp(seed=1).state_dict())


def _mul(ac):
    with torch.no_grad():
        ac.pi_net[0].weight.mul_(1.5)


def _copy(ac):
    with torch.no_grad():
        ac.v_net[2].bias.copy_(torch.ones(256))


def _data_swap(ac):
    p = ac.pi_net[2].weight
    version = p._version
    p.data = torch.randn_like(p)      # new storage, same version counter
    assert p._version == version


CHANGES = {"optimizer_step": _optimizer_step, "load_state_dict": _load_other, "mul_": _mul, "copy_": _copy,
           "data_swap": _data_swap}


@pytest.mark.parametrize("kind", sorted(CHANGES))
def test_plan_is_rebuilt_exactly_once_after_a_parameter_change(kind):
    ac, build = _mlp(), Counter()
    first = _get(ac, build)
    assert build.calls == 1 and build.prev == [None]          # the first build has no previous value
    assert _get(ac, build) is first and build.calls == 1
    CHANGES[kind](ac)
    second = _get(ac, build)
    assert build.calls == 2, kind
    assert build.prev[1] is first                             # a rebuild is handed the value it replaces
    assert second is not first
    assert _get(ac, build) is second and _get(ac, build) is second and build.calls == 2


def test_every_change_in_a_row_rebuilds_once_each():
    ac, build = _mlp(), Counter()
    _get(ac, build)
    for n, kind in enumerate(sorted(CHANGES), start=2):
        CHANGES[kind](ac)
        out = _get(ac, build)
        assert build.calls == n and out == {"n": n}, kind
        assert build.prev[-1] == {"n": n - 1}
        assert _get(ac, build) is out and build.calls == n


def test_plan_is_not_rebuilt_by_what_leaves_the_values_alone():
    ac, build = _mlp(), Counter()
    first = _get(ac, build)
    _loss(ac).backward()                                      # forward + backward: gradients, not values
    assert _get(ac, build) is first
    for set_to_none in (False, True):
        _loss(ac).backward()
        torch.optim.Adam(ac.parameters()).zero_grad(set_to_none=set_to_none)
        ac.zero_grad(set_to_none=set_to_none)
        assert _get(ac, build) is first
    with torch.no_grad():                                     # reading
        sum(float(p.sum()) for p in ac.parameters())
        [p.detach().clone() for p in ac.parameters()]
        ac.state_dict()
        ac.pi_net[0].weight.double()
    ac.eval(); ac.train()
    assert _get(ac, build) is first and build.calls == 1


def test_another_tag_is_another_plan():
    ac, build = _mlp(), Counter()
    a = _get(ac, build, tag=torch.float32)
    assert _get(ac, build, tag=torch.float32) is a and build.calls == 1
    b = _get(ac, build, tag=torch.bfloat16)
    assert build.calls == 2 and b is not a
    assert build.prev[1] is a                                 # one slot per attribute: the other tag's value is replaced
    assert _get(ac, build, tag=torch.bfloat16) is b and build.calls == 2
    _get(ac, build, tag=torch.float32)
    assert build.calls == 3


def test_fused_plan_follows_the_parameters():
    """The library-GEMM modes' plan (fused_plan) holds COPIES of the weights: after each kind of change they are the
    current values."""
    for make, layer in ((_mlp, lambda ac: ac.pi_net[2]), (_rnn, lambda ac: ac.pi.net_out[2])):
        ac = make()
        plan = ac.fused_plan(torch.float32)
        assert plan is not None and ac.fused_plan(torch.float32) is plan
        lin = layer(ac)
        with torch.no_grad():
            lin.weight.mul_(2.0)
        plan2 = ac.fused_plan(torch.float32)
        assert plan2 is not plan and torch.equal(plan2["mid"][0][0], lin.weight)
        lin.weight.data = torch.full_like(lin.weight, 0.25)
        assert torch.equal(ac.fused_plan(torch.float32)["mid"][0][0], lin.weight)
        assert ac.fused_plan(torch.bfloat16)["mid"][0][0].dtype == torch.bfloat16


def test_cast_cached_follows_version_and_storage():
    ac = _mlp()
    p = ac.pi_net[0].weight
    assert P._cast_cached(p, torch.float32) is p              # same dtype: the parameter itself
    c = P._cast_cached(p, torch.bfloat16)
    assert c.dtype == torch.bfloat16 and torch.equal(c, p.detach().to(torch.bfloat16))
    assert P._cast_cached(p, torch.bfloat16) is c
    assert P._cast_cached(p, torch.float64) is not c and P._cast_cached(p, torch.bfloat16) is c   # one entry per dtype
    _loss(ac).backward()
    ac.zero_grad()
    assert P._cast_cached(p, torch.bfloat16) is c             # gradients leave it alone
    with torch.no_grad():
        p.mul_(3.0)                                           # version bump
    c2 = P._cast_cached(p, torch.bfloat16)
    assert c2 is not c and torch.equal(c2, p.detach().to(torch.bfloat16)) and not torch.equal(c2, c)
    version = p._version
    p.data = torch.randn_like(p)                              # storage change at the same version
    assert p._version == version
    c3 = P._cast_cached(p, torch.bfloat16)
    assert c3 is not c2 and torch.equal(c3, p.detach().to(torch.bfloat16))
    assert P._cast_cached(p, torch.bfloat16) is c3


def test_cast_cached_entry_dies_with_its_parameter():
    """CPython hands the id of a freed object to the next one of its size: a second model built after the first was
    freed must never be served the first's cast."""
    before = len(P._CAST_CACHE)
    for seed in range(6):                                     # (several rounds: id reuse is likely, not certain)
        ac = _mlp(seed)
        params = [ac.pi_net[0].weight, ac.pi_net[0].bias, ac.v_net[4].weight]
        casts = [P._cast_cached(p, torch.bfloat16) for p in params]
        for p, c in zip(params, casts):
            assert torch.equal(c, p.detach().to(torch.bfloat16)), seed
        assert len(P._CAST_CACHE) == before + len(params)
        del ac, params, p
        gc.collect()
        assert len(P._CAST_CACHE) == before, seed            # the entries left with their parameters
        del casts, c


def test_cast_cached_does_not_trust_a_reused_id():
    """The same, with the id collision forced: an entry filed under another parameter's id is not served."""
    a, b = _mlp(0).pi_net[0].weight, _mlp(1).pi_net[0].weight
    ca = P._cast_cached(a, torch.bfloat16)
    key_a, key_b = (id(a), torch.bfloat16), (id(b), torch.bfloat16)
    P._CAST_CACHE[key_b] = P._CAST_CACHE[key_a]               # what a reused id would find
    try:
        cb = P._cast_cached(b, torch.bfloat16)
        assert cb is not ca and torch.equal(cb, b.detach().to(torch.bfloat16))
    finally:
        P._CAST_CACHE.pop(key_b, None)


def test_device_blobs_are_none_on_cpu_modules():
    """The contract multi_ppo._fused_mode relies on: no packed blob for modules that are not on a GPU."""
    m, r = _mlp(), _rnn()
    assert m.mlp_blob() is None and m.mlp_blob("bf16") is None and m.mlp_blob("x3") is None
    assert r.zero_vo_plan() is None and r.rnn_tiles_blob() is None
    assert _rnn(mode="LSTM").zero_vo_plan() is None and _rnn(mode="LSTM").rnn_tiles_blob() is None
    with pytest.raises(ValueError):
        m.mlp_blob("fp8")
    assert m.fused_plan(torch.float32) is not None            # (the library-GEMM plan is plain tensors: any device)


def test_kernel_policy_step_fits_no_cpu_module():
    """The launcher's predicate is the models' own: nothing fits off the GPU, whatever the kind; a refusal starts with
    the caller's words for what was asked; a kind that does not exist is an error, not a misfit."""
    for ac, width in ((_mlp(), 30), (_rnn(), 102), (_rnn(mode="LSTM"), 102)):
        for kind in KernelPolicyStep.KINDS:
            assert KernelPolicyStep.fits(ac, kind, width) is False, kind
            with pytest.raises(ValueError) as ex:
                KernelPolicyStep(ac, kind, width, 64, option=f"policy_kernel={kind!r}")
            assert str(ex.value).startswith(f"policy_kernel={kind!r} needs "), str(ex.value)
        for call in (lambda: KernelPolicyStep.fits(ac, "gemm", width), lambda: KernelPolicyStep(ac, "gemm", width, 64)):
            with pytest.raises(ValueError, match="kind must be one of"):
                call()
    assert set(KernelPolicyStep.KINDS) == {"mlp", "mlp_x3", "rnn0", "rnn_tiles", "rnn_tiles_x3"}
