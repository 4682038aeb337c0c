"""The action noise of every rollout against an independent statement of its generator.

normal3 (csrc/rvo3d_rollout_kernels.hpp) is Philox4x32-10 with counter (row, step) and key seed, then Box-Muller in
fast float32 intrinsics; every sampling kernel reaches it through finish_row.  tests/philox_ref.py states the same in
numpy integers and float64 and is itself pinned to the published known answers (CPU test below).  On the GPU:
rvo3d_policy_sample in direct mode (hidden 0, mu 0, log_std 0, std_factor 1) must give raw = sd * eps_ref for every
(seed, step) of SEEDS x STEPS - both words of both, rows beyond 2^16 - the device counter must add to `step` with the
carry into its high word, and the two heads kernels must draw the same stream.  The MLP, x3, tiles and rows kernels are
tied to direct mode by their own tests, which pins the stream of every sampling kernel.

Tolerance of the comparison with float64 Box-Muller: a wrong stream differs like two independent normals do (half of
the elements by more than 0.9), so any bound up to 1e-2 separates right from wrong.  Measured on an MI355X over the 20
(seed, step) pairs x 70 001 rows x 3: max |raw - sd * eps_ref| = 1.990e-06 (1.43e-06 .. 1.99e-06 per pair: the fast
log, sincos and sqrt of normal3, plus the float32 roundings of r * c and sd * eps); asserted: four times that, 7.96e-06."""
import ctypes as C

import numpy as np
import pytest

import philox_ref

ROWS = 70001                                    # past 2^16, not a multiple of 256 (the direct kernel's workgroup)
SEEDS = (0, 7, 2 ** 32 + 7, 2 ** 64 - 1)
STEPS = (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63)
MEASURED_MAX = 1.990e-06                        # max |raw - sd * eps_ref| over SEEDS x STEPS, measured on an MI355X
TOL = 4 * MEASURED_MAX


def test_philox_reference_gives_the_published_known_answers():
    for ctr, key, want in philox_ref.KNOWN_ANSWERS:
        got = philox_ref.philox4x32(ctr, key)
        assert [int(w) for w in got] == list(want), [hex(int(w)) for w in got]
    # vectorised over the counter: the same words as one call per counter
    ctrs = np.array([k[0] for k in philox_ref.KNOWN_ANSWERS[1:]], dtype=np.uint64)
    for j, (_, key, want) in enumerate(philox_ref.KNOWN_ANSWERS[1:]):
        got = philox_ref.philox4x32(tuple(ctrs[:, i] for i in range(4)), key)
        assert [int(w[j]) for w in got] == list(want)
    # the stream's layout: (row, step) and (step, row) are different counters; every word of step and seed counts
    a = philox_ref.normal3_ref(7, 3, 8)
    assert not np.array_equal(a[3], philox_ref.normal3_ref(7, 3 + 2 ** 32, 8)[3])
    assert not np.array_equal(a[3], philox_ref.normal3_ref(7 + 2 ** 32, 3, 8)[3])
    assert not np.array_equal(philox_ref.normal3_ref(7, 3, 8)[5], philox_ref.normal3_ref(7, 5, 8)[3])
    assert np.isfinite(a).all()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _direct(rows, seed, step, log_std=None, mu=None):
    """rvo3d_policy_sample in direct mode on zero heads: (act, raw) as numpy float32."""
    import torch
    from rvo3d_amd import _lib
    dev = "cuda"
    mu = torch.zeros((rows, 3), device=dev) if mu is None else mu
    v = torch.zeros((rows, 1), device=dev)
    log_std = torch.zeros(3, device=dev) if log_std is None else log_std
    act, raw = torch.full((rows, 3), 9.0, device=dev), torch.full((rows, 3), 9.0, device=dev)
    logp, val = torch.full((rows,), 9.0, device=dev), torch.full((rows,), 9.0, device=dev)
    hd = _lib.PolicyHeads(mu.data_ptr(), v.data_ptr(), 3, 1, _lib.RVO3D_F32, 0, 0, 0, None, None, None, None,
                          log_std.data_ptr())
    _lib.check(_lib.lib().rvo3d_policy_sample(C.byref(hd), rows, 1.0, seed, step, _p(act), _p(logp), _p(val), None,
                                              _p(raw), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "rvo3d_policy_sample")
    torch.cuda.synchronize()
    return act.cpu().numpy(), raw.cpu().numpy()


# std = clamp(std_factor * exp(log_std) + 1e-6, 1e-4, 10) at log_std 0, std_factor 1, in float32 as sample_consts forms it
SD = np.float32(1.0) + np.float32(1e-6)


@pytest.mark.gpu
def test_direct_mode_noise_is_philox_box_muller():
    """Measured on an MI355X: max |raw - sd * eps_ref| over all 20 pairs = 1.990e-06; the bound is four times that."""
    worst = 0.0
    for seed in SEEDS:
        for step in STEPS:
            act, raw = _direct(ROWS, seed, step)
            want = float(SD) * philox_ref.normal3_ref(seed, step, ROWS)
            assert np.isfinite(raw).all()
            err = float(np.abs(raw.astype(np.float64) - want).max())
            print(f"seed {seed:#x} step {step:#x}: max |raw - sd eps_ref| = {err:.3e}")
            worst = max(worst, err)
            assert np.isfinite((raw / SD)).all()
            assert np.array_equal(act, np.round(raw, 2))         # np.round(a, 2) in numpy's own float32 arithmetic
            assert err <= TOL, (hex(seed), hex(step), err)
    print(f"max over all pairs: {worst:.3e}")


@pytest.mark.gpu
@pytest.mark.parametrize("s,k", [(5, 3), (2 ** 32 - 1, 1)])
def test_device_counter_adds_to_the_step_with_carry(s, k):
    """With the process-wide counter set to k, a call with base step s is bit for bit the call with step s + k and no
    counter - also where the sum carries into the high word."""
    import torch
    from rvo3d_amd import _lib
    L = _lib.lib()
    rows = 1000
    _, plain = _direct(rows, 11, s + k)
    _, base = _direct(rows, 11, s)
    ctr = torch.tensor([k], dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    try:
        _lib.check(L.rvo3d_rollout_set_step_counter(_p(ctr)), "rvo3d_rollout_set_step_counter")
        _, counted = _direct(rows, 11, s)
    finally:
        rc = L.rvo3d_rollout_set_step_counter(None)
    assert rc == 0
    assert int(ctr[0]) == k                                      # a sampling launch reads the counter, never writes it
    assert counted.tobytes() == plain.tobytes()
    assert counted.tobytes() != base.tobytes()
    assert _direct(rows, 11, s)[1].tobytes() == base.tobytes()   # no counter left behind
    want = float(SD) * philox_ref.normal3_ref(11, s + k, rows)
    assert float(np.abs(counted - want).max()) <= TOL


@pytest.mark.gpu
@pytest.mark.parametrize("dt,hidden", [("float32", 128), ("bfloat16", 256)])
def test_heads_kernels_draw_the_same_stream(dt, hidden):
    """policy_sample_kernel<float, 1> / <bf16_t, 1>: (raw - mu) / sd is the direct-mode noise of the same (seed, step,
    row), to the float32 rounding of that expression (raw = mu + sd eps with |raw| < 8: half an ulp of 4.8e-7 for the sum,
    as much for the difference; the suite's bound for this comparison is 1e-6, test_policy_mlp_sample_matches_torch)."""
    import torch
    from rvo3d_amd import _lib
    from test_gpu_rollout import _sample
    rows, seed, step = 64 * 3 + 37, 2 ** 32 + 7, 2 ** 32
    tdt = getattr(torch, dt)
    g = torch.Generator(device="cuda").manual_seed(hidden)
    H2 = torch.relu(torch.randn((rows, 2 * hidden), device="cuda", generator=g)).to(tdt)
    wpi = torch.randn((3, hidden), device="cuda", generator=g) * 0.08
    bpi = torch.randn(3, device="cuda", generator=g) * 0.1
    wv = torch.randn(hidden, device="cuda", generator=g) * 0.08
    bv = torch.randn(1, device="cuda", generator=g)
    log_std = torch.zeros(3, device="cuda")
    code = _lib.RVO3D_BF16 if tdt == torch.bfloat16 else _lib.RVO3D_F32
    _, _, _, mu, raw = _sample(H2[:, :hidden], H2[:, hidden:], wpi, bpi, wv, bv, log_std, rows, hidden, code,
                               seed=seed, step=step)
    mu, raw = mu.cpu().numpy(), raw.cpu().numpy()
    assert np.abs(mu).max() < 1 and np.abs(mu).max() > 0.1       # real heads: tanh of something
    _, raw_d = _direct(rows, seed, step)
    eps_k, eps_d = (raw - mu) / SD, raw_d / SD
    assert np.isfinite(eps_k).all()
    np.testing.assert_allclose(eps_k, eps_d, atol=1e-6, rtol=0)
    # and that is the reference's stream, not merely the same one twice
    want = philox_ref.normal3_ref(seed, step, rows)
    assert float(np.abs(eps_d - want).max()) <= TOL
