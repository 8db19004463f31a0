"""The duration posterior's host surface (no GPU needed): both libraries export the new symbols,
the headers declare them, the workspace query is a pure, monotone function of the shape, and
ssnt_duration_class_targets (pure torch) on CPU tensors."""
import numpy as np
import pytest
import torch

from test_capi_exports import AB_HEADER, AB_LIB, HEADER, LIB, _exported, header_functions

SYMBOLS = ("ssnt_duration_posterior_workspace_size", "ssnt_duration_posterior_device")
AB_SYMBOLS = ("ssnt_duration_posterior_block", "ssnt_duration_posterior_sweep_rows",
              "ssnt_duration_posterior_launches")


def test_symbols_declared_and_exported():
    fns, ab_fns = header_functions(HEADER), header_functions(AB_HEADER)
    exported, ab_exported = _exported(LIB), _exported(AB_LIB)
    for s in SYMBOLS:
        assert s in fns and s in exported and s in ab_exported, s
    for s in AB_SYMBOLS:
        assert s in ab_fns and s in ab_exported and s not in exported, s


def test_workspace_size_is_a_monotone_function_of_the_shape():
    from ssnt_tts_amd._lib import load
    size = load().ssnt_duration_posterior_workspace_size
    base = (3, 40, 70, 16)
    w = size(*base)
    assert w > 0 and w == size(*base)  # (no state: the same answer twice)
    # alpha's and beta's rows, 8 B per cell and direction, lie inside it
    assert w >= 2 * 3 * 40 * 70 * 8
    for i in range(4):
        prev = w
        for step in (1, 2, 7, 64):
            a = list(base)
            a[i] += step
            cur = size(*a)
            assert cur >= prev, (i, step)
            prev = cur
    assert size(4, 40, 70, 16) > w and size(3, 41, 70, 16) > w and size(3, 40, 129, 16) > w
    for bad in ((0, 40, 70, 16), (3, 40, 1025, 16), (3, 40, 70, 1), (3, 40, 70, 257), (3, -1, 70, 16)):
        assert size(*bad) == 0, bad


def test_block_query():
    from ssnt_tts_amd._lib import load_ab
    ab = load_ab()
    for U, D, obs in ((1, 2, 0), (80, 32, 1), (1024, 256, 1)):
        blk = ab.ssnt_duration_posterior_block(U, D, obs)
        rows, tile = blk & 0xFFFF, blk >> 16
        assert rows >= 1 and tile >= 1
        assert ab.ssnt_duration_posterior_sweep_rows(U, obs) >= 1
    assert ab.ssnt_duration_posterior_sweep_rows(1025, 0) == 0
    assert ab.ssnt_duration_posterior_block(1025, 8, 0) == 0
    assert ab.ssnt_duration_posterior_block(8, 1, 0) == 0
    assert ab.ssnt_duration_posterior_launches(0) != 0 and ab.ssnt_duration_posterior_launches(4) != 0
    assert ab.ssnt_duration_posterior_launches(3) == 0


def _dur_post(B=2, U=3, D=6, seed=0):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.dirichlet(np.ones(D), size=(B, U)).astype(np.float32))


def test_class_targets_gather():
    import ssnt_tts_amd as S
    dp = _dur_post()
    table = [0, 3, 1, 4, 5, 9, 2]  # 5 = D-1 is the tail bin, 9 lies beyond it
    targets, residual = S.ssnt_duration_class_targets(dp, table)
    assert targets.shape == (2, 3, 7) and residual.shape == (2, 3)
    for i, d in enumerate(table):
        want = dp[..., d] if d < 5 else torch.zeros(2, 3)
        assert torch.equal(targets[..., i], want), (i, d)
    # the tail's mass is what no class represents
    assert torch.allclose(residual, dp[..., 5], atol=1e-6)
    assert torch.allclose(targets.sum(-1) + residual, dp.sum(-1), atol=1e-6)
    # BASELINE's v2 table [0..15] over 17 bins: class index = duration, the residual is the tail
    dp = _dur_post(D=17, seed=1)
    targets, residual = S.ssnt_duration_class_targets(dp, torch.arange(16))
    assert torch.equal(targets, dp[..., :16]) and torch.allclose(residual, dp[..., 16], atol=1e-6)
    # a table that misses durations: their mass is in the residual
    targets, residual = S.ssnt_duration_class_targets(dp, [1, 2])
    assert torch.allclose(targets.sum(-1) + residual, dp.sum(-1), atol=1e-6)
    assert torch.allclose(residual, dp.sum(-1) - dp[..., 1] - dp[..., 2], atol=1e-6)


def test_class_targets_refuses_repeats_and_bad_input():
    import ssnt_tts_amd as S
    dp = _dur_post()
    with pytest.raises(ValueError):
        S.ssnt_duration_class_targets(dp, [1, 2, 2])
    with pytest.raises(ValueError):
        S.ssnt_duration_class_targets(dp, [1, -1])
    with pytest.raises(ValueError):
        S.ssnt_duration_class_targets(dp[0], [1, 2])
