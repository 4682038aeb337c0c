"""Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) in plain numpy
integer arithmetic, written from the algorithm's definition, and the rollout kernels' use of it (normal3 in
csrc/rvo3d_rollout_kernels.hpp) restated on top: a helper of tests/test_gpu_noise_stream.py, not a test module.

One round maps the counter (c0, c1, c2, c3) under the key (k0, k1) to
    (hi(M1 c2) ^ c1 ^ k0,  lo(M1 c2),  hi(M0 c0) ^ c3 ^ k1,  lo(M0 c0))
with the 32 x 32 -> 64 bit products split into their high and low words; the key is bumped by (W0, W1) between rounds
(not after the last)."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57      # multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85      # key increments (golden ratio, sqrt(3) - 1)
ROUNDS = 10
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)

# published known answers (Random123's kat_vectors, philox4x32 10): counter words, key words, output words
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def _words(x):
    """An integer (Python int of any size below 2^64, or an array of them) as (low, high) 32-bit words in uint64."""
    x = np.asarray(x, dtype=np.uint64)
    return x & _MASK, x >> _S32


def philox4x32(counter, key, rounds=ROUNDS):
    """counter: four 32-bit words, key: two (scalars or arrays that broadcast).  Returns four uint32 arrays."""
    c = [np.asarray(w, dtype=np.uint64) for w in counter]
    k = [np.asarray(w, dtype=np.uint64) for w in key]
    assert all((w <= _MASK).all() for w in c + k), "32-bit words"
    for r in range(rounds):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]           # < 2^64: exact in uint64
        c = [(p1 >> _S32) ^ c[1] ^ k[0], p1 & _MASK, (p0 >> _S32) ^ c[3] ^ k[1], p0 & _MASK]
        if r + 1 < rounds:
            k = [(k[0] + np.uint64(W0)) & _MASK, (k[1] + np.uint64(W1)) & _MASK]
    return [w.astype(np.uint32) for w in np.broadcast_arrays(*c)]


def uniforms(seed, step, rows):
    """The four float32 uniforms of rows 0 .. rows-1: counter (row low, row high, step low, step high), key (seed low,
    seed high); u = (float32(x) + 0.5f) * 2^-32 in float32 arithmetic (the conversion rounds to nearest even, so the
    top values of x give u = 1)."""
    r_lo, r_hi = _words(np.arange(rows, dtype=np.uint64))
    s_lo, s_hi = _words(step)
    k_lo, k_hi = _words(seed)
    x = philox4x32((r_lo, r_hi, s_lo, s_hi), (k_lo, k_hi))
    return [(w.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -32) for w in x]


def normal3_ref(seed, step, rows):
    """eps [rows, 3] float64: Box-Muller on the uniforms above.  float32 up to the arguments of log and sincos (u = 1
    becomes 0.99999994, the angle is float32(6.2831855f * u)), float64 from there on."""
    u = uniforms(seed, step, rows)
    assert all(w.dtype == np.float32 for w in u)
    top = np.float32(0.99999994)
    u0, u2 = (np.where(w < np.float32(1.0), w, top).astype(np.float64) for w in (u[0], u[2]))
    a1, a3 = ((np.float32(6.2831855) * w).astype(np.float64) for w in (u[1], u[3]))
    assert (np.float32(6.2831855) * u[1]).dtype == np.float32
    r0, r1 = np.sqrt(-2.0 * np.log(u0)), np.sqrt(-2.0 * np.log(u2))
    return np.stack([r0 * np.cos(a1), r0 * np.sin(a1), r1 * np.cos(a3)], axis=-1)
