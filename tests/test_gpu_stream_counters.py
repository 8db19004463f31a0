"""Streaming fwd-bwd: the LDS progress counters (row numbers, one wide read per poll, one 8-byte
publish) across every ring wrap, half-block size and cut position, on the product library.

Bar: loss, grad (and grad_obs) and the fused loss_sum BIT-EXACT against the split-exponent C
oracle, with status word 0 (a counter off by one shows as the bounded-spin timeout bit, not as a
wrong number). Ragged batches: step_len takes every value 1..48 once, so the chains meet every
ring wrap (R = 8 / 4, the chain-row ring), both half-block sizes (4 and 2), the cut at
M = 0, 1, 2 and utterances shorter than the converter prefetch depth; one row per batch is
infeasible (S < P).
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F_TERM = 1
B, T = 48, 48
# U -> the instance the product dispatch must pick
INSTANCES = {
    80: ("K=2", "NC=3,NH=4", "NV=0"),   # the headline's instance, 16 waves
    64: ("K=1", "NC=3,NH=4", "NV=0"),
    81: ("K=2", "NC=3,NH=4", "NV=1"),   # narrow form
    160: ("K=4", "NC=2,NH=2", "NV=0"),  # 10 waves: the 8-byte counter read
}


def _wave_order_sum(loss):
    """The library's fixed summation order: 64 lane-strided f32 partial sums, then an xor
    butterfly (lattice_dev.h wave_loss_sum)."""
    acc = np.zeros(64, np.float32)
    with np.errstate(invalid="ignore"):
        for i, v in enumerate(np.asarray(loss, np.float32)):
            acc[i % 64] = np.float32(acc[i % 64] + v)
        off = 32
        while off >= 1:
            acc = (acc + acc[np.arange(64) ^ off]).astype(np.float32)
            off //= 2
    return acc[0]


@functools.lru_cache(maxsize=None)
def _ragged_case(U, obs, flags):
    """Inputs and the oracle's outputs, computed once per case and shared (read-only)."""
    import oracle as O
    rng = np.random.default_rng(1000 * U + 2 * int(obs) + flags)
    S = rng.permutation(np.arange(1, T + 1)).astype(np.int32)  # every length 1..48 once
    P = np.array([rng.integers(1, min(s, U) + 1) for s in S], np.int32)
    bad = int(np.argmax(S == 30))
    P[bad] = 31  # infeasible: S < P
    lt = O.synth_log_trans(B, T, U, seed=U + flags)
    lo = (rng.standard_normal((B, T, U)) * 15 - 40).astype(np.float32) if obs else None
    o = O.fwd_bwd_xf(lt, S, P, log_obs=lo, flags=flags)
    for v in (lt, lo, S, P, *o.values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return lt, lo, S, P, bad, o


def _run(gpu, lt, lo, S, P, flags):
    dev = torch.device("cuda:0")
    r = gpu.ssnt_fwd_bwd(torch.tensor(lt, device=dev), torch.tensor(S, device=dev),
                         torch.tensor(P, device=dev), None if lo is None else torch.tensor(lo, device=dev),
                         terminal_emit=bool(flags & F_TERM), loss_sum=True, check=False)
    return {k: v.cpu().numpy() for k, v in r.items()}


def _check(gpu, g, o, U, obs):
    name = gpu.last_fwd_bwd_kernel()
    assert name.startswith("k_fwd_bwd_stream<"), name
    for part in INSTANCES[U] + (f"OBS={int(obs)}",):
        assert part in name, (part, name)
    assert int(g["status"].item()) == 0, f"status word {int(g['status'].item()):#x} ({name})"
    keys = ["loss", "grad"] + (["grad_obs"] if obs else [])
    for k in keys:
        assert g[k].shape == o[k].shape, k
        assert g[k].tobytes() == np.ascontiguousarray(o[k]).tobytes(), \
            f"{k}: {int(np.sum(g[k] != o[k]))} values differ ({name})"
    want = _wave_order_sum(o["loss"])
    assert np.float32(g["loss_sum"][0]).tobytes() == np.float32(want).tobytes(), (g["loss_sum"][0], want)


@pytest.mark.parametrize("flags", [F_TERM, 0], ids=["term", "noterm"])
@pytest.mark.parametrize("obs", [False, True], ids=["plain", "obs"])
@pytest.mark.parametrize("U", sorted(INSTANCES))
def test_ragged_every_length_bit_exact(gpu, U, obs, flags):
    lt, lo, S, P, bad, o = _ragged_case(U, obs, flags)
    g = _run(gpu, lt, lo, S, P, flags)
    _check(gpu, g, o, U, obs)
    # the infeasible row, exactly as before: +inf loss, zero gradient
    assert np.isposinf(g["loss"][bad]) and not g["grad"][bad].any()
    if obs:
        assert not g["grad_obs"][bad].any()


def test_full_lengths_headline_row_count(gpu, oracle):
    # the workload's row count at a small batch: the LDS storage plan equals the headline's
    Bf, Tf, U = 8, 200, 80
    lt = oracle.synth_log_trans(Bf, Tf, U, seed=3)
    S, P = np.full(Bf, Tf, np.int32), np.full(Bf, U, np.int32)
    o = oracle.fwd_bwd_xf(lt, S, P, flags=F_TERM)
    g = _run(gpu, lt, None, S, P, F_TERM)
    _check(gpu, g, o, U, False)
    assert "LDS=1" in gpu.last_fwd_bwd_kernel(), gpu.last_fwd_bwd_kernel()
