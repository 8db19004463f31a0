"""The banded lattice's Python layer on CPU tensors (no GPU): the pure-torch band helpers, the
refusals of ssnt_fwd_bwd_band, and the order of its arguments with a stub in place of the library,
as tests/test_call_protocol.py does for the shared protocol."""
import ctypes

import numpy as np
import pytest
import torch

import band_ref as BR
import ssnt_tts_amd as S


def _random_alignment(rng, T, s, p):
    """position (T,) of a monotone alignment 0 -> p-1 over s steps; -1 beyond."""
    pos = np.full(T, -1, np.int64)
    moves = np.zeros(max(s - 1, 0), np.int64)
    moves[rng.choice(max(s - 1, 1), size=p - 1, replace=False) if p > 1 else []] = 1
    pos[:s] = np.concatenate([[0], np.cumsum(moves)])
    return pos


@pytest.mark.parametrize("width", [1, 2, 3, 4, 7, 8])
def test_band_from_positions_is_valid_and_contains_the_path(width):
    rng = np.random.default_rng(width)
    T = 24
    # P < R, P = R + 1, S = P, S = 1 and ragged ones
    SP = [(24, max(width - 1, 1)), (24, width + 1), (13, 13), (1, 1), (20, 9), (24, 24), (17, width), (2, 2), (2, 1)]
    pos = np.stack([_random_alignment(rng, T, s, p) for s, p in SP])
    sl = torch.tensor([s for s, _ in SP])
    pl = torch.tensor([p for _, p in SP])
    bs = S.ssnt_band_from_positions(torch.from_numpy(pos), sl, pl, width)
    assert bs.dtype == torch.int32 and tuple(bs.shape) == pos.shape
    for b, (s, p) in enumerate(SP):
        row = bs[b].numpy()
        assert BR.is_valid(row, s, p, width), (s, p, row)
        assert np.all((row[:s] <= pos[b, :s]) & (pos[b, :s] < row[:s] + width))
        assert np.all(row[s:] == row[s - 1])
        want = np.clip(pos[b, :s] - width // 2, 0, max(p - width, 0))
        assert np.array_equal(row[:s], want)
    # int32 positions, list lengths
    again = S.ssnt_band_from_positions(torch.from_numpy(pos).to(torch.int32), [s for s, _ in SP],
                                       [p for _, p in SP], width)
    assert torch.equal(again, bs)


def test_gather_scatter_round_trip():
    rng = np.random.default_rng(0)
    B, T, U, R = 3, 9, 11, 4
    bs = np.stack([BR.make_band("random", T, T, U if b else 6, R, rng) for b in range(B)])
    bs[2, 5:] += 20  # windows that leave the tensor entirely
    bst = torch.from_numpy(bs)
    for tail in ((), (2,)):
        dense = torch.from_numpy(rng.standard_normal((B, T, U) + tail).astype(np.float32))
        band = S.ssnt_band_gather(dense, bst, R, float("-inf"))
        assert tuple(band.shape) == (B, T, R) + tail
        assert np.array_equal(band.numpy(), BR.gather(dense.numpy(), bs, R, fill=-np.inf))
        back = S.ssnt_band_scatter(band, bst, U, fill=7.0)
        idx = bs[:, :, None] + np.arange(R)
        inside = np.zeros((B, T, U), bool)
        for b in range(B):
            for s in range(T):
                inside[b, s, idx[b, s][(idx[b, s] >= 0) & (idx[b, s] < U)]] = True
        assert np.array_equal(back.numpy()[inside], dense.numpy()[inside])
        assert np.all(back.numpy()[~inside] == 7.0)
        assert torch.equal(S.ssnt_band_gather(back, bst, R, float("-inf")), band)
    # negative starts gather the fill and scatter nothing
    neg = torch.full((B, T), -R, dtype=torch.int32)
    dense = torch.ones((B, T, U))
    assert torch.all(S.ssnt_band_gather(dense, neg, R, 5.0) == 5.0)
    assert torch.all(S.ssnt_band_scatter(torch.ones((B, T, R)), neg, U) == 0)
    ints = torch.arange(B * T * U).reshape(B, T, U)
    assert S.ssnt_band_gather(ints, bst, R, -1).dtype == torch.int64


def test_helpers_refuse_wrong_shapes_and_dtypes():
    dense, bs = torch.zeros((2, 5, 6, 2)), torch.zeros((2, 5), dtype=torch.int32)
    with pytest.raises(TypeError):
        S.ssnt_band_gather(dense, bs.float(), 3, 0.0)
    with pytest.raises(ValueError):
        S.ssnt_band_gather(dense, bs[:, :4], 3, 0.0)
    with pytest.raises(ValueError):
        S.ssnt_band_gather(dense, bs, 0, 0.0)
    with pytest.raises(ValueError):
        S.ssnt_band_gather(torch.zeros((2, 5)), bs, 3, 0.0)
    with pytest.raises(TypeError):
        S.ssnt_band_scatter(torch.zeros((2, 5, 3)), bs.double(), 6)
    with pytest.raises(ValueError):
        S.ssnt_band_scatter(torch.zeros((2, 4, 3)), bs, 6)
    with pytest.raises(ValueError):
        S.ssnt_band_scatter(torch.zeros((2, 5, 3)), bs, -1)
    with pytest.raises(TypeError):
        S.ssnt_band_from_positions(torch.zeros((2, 5)), [5, 5], [2, 2], 3)
    with pytest.raises(ValueError):
        S.ssnt_band_from_positions(torch.zeros(5, dtype=torch.int32), [5], [2], 3)
    with pytest.raises(ValueError):
        S.ssnt_band_from_positions(torch.zeros((2, 5), dtype=torch.int32), [5, 5], [2, 2], 0)


class StubLib:
    """Stands in for the library: records what the two band symbols receive."""

    def __init__(self, ws_bytes):
        self.ws_bytes, self.query, self.args, self.status_at_call = ws_bytes, None, None, None

    def ssnt_fwd_bwd_band_workspace_size(self, *shape):
        self.query = shape
        return self.ws_bytes

    def ssnt_fwd_bwd_band_device(self, *args):
        self.args = args
        self.status_at_call = ctypes.cast(args[14], ctypes.POINTER(ctypes.c_int))[0]
        return 0

    def ssnt_status_from_bits(self, bits):
        return 0


@pytest.fixture
def cpu(monkeypatch):
    monkeypatch.setattr(S, "_stream", lambda dev: None)
    monkeypatch.setattr(S, "_dev", lambda t, dtype, name: t.to(dtype).contiguous())
    return torch.device("cpu")


def test_fwd_bwd_band_argument_order(cpu, monkeypatch):
    from ssnt_tts_amd._lib import SIGNATURES
    B, T, R = 2, 6, 3
    lt, lo = torch.zeros((B, T, R, 2)), torch.zeros((B, T, R))
    bs = torch.zeros((B, T), dtype=torch.int64)
    sl, pl = torch.tensor([6, 5], dtype=torch.int32), torch.tensor([2, 3], dtype=torch.int32)
    stub = StubLib(40)
    monkeypatch.setattr(S, "load", lambda require_gpu=False: stub)
    mine = torch.empty((B,))
    r = S.ssnt_fwd_bwd_band(lt, bs, sl, pl, lo, zero_infinity=True, out={"loss": mine})
    a = stub.args
    assert len(a) == len(SIGNATURES["ssnt_fwd_bwd_band_device"][1]) == 16
    assert stub.query == (B, T, R)
    assert a[0] == lt.data_ptr() and a[1] == lo.data_ptr() and a[3] == sl.data_ptr() and a[4] == pl.data_ptr()
    assert a[2] not in (None, bs.data_ptr())  # converted to i32
    assert a[5:9] == (B, T, R, S.FLAG_TERMINAL_EMIT | S.FLAG_ZERO_INFINITY)
    assert a[9] == mine.data_ptr() and r["loss"] is mine
    assert a[10] == r["grad"].data_ptr() and tuple(r["grad"].shape) == (B, T, R, 2)
    assert a[11] == r["grad_obs"].data_ptr() and tuple(r["grad_obs"].shape) == (B, T, R)
    assert a[12] is not None and a[13] == 40
    assert a[14] == r["status"].data_ptr() and stub.status_at_call == 0 and a[15] is None
    # no gradient: no workspace query, NULL gradients; no log_obs: NULL and no grad_obs
    stub2 = StubLib(40)
    monkeypatch.setattr(S, "load", lambda require_gpu=False: stub2)
    r = S.ssnt_fwd_bwd_band(lt, bs.to(torch.int32), sl, pl, terminal_emit=False, need_grad=False)
    a = stub2.args
    assert stub2.query is None and a[1] is None and a[2] is not None and a[8] == 0
    assert a[10] is None and a[11] is None and a[12] is None and a[13] == 0
    assert set(r) == {"loss", "status"}
    r = S.ssnt_fwd_bwd_band(lt, bs, sl, pl)
    assert set(r) == {"loss", "grad", "status"} and stub2.args[11] is None


def test_fwd_bwd_band_refusals(cpu, monkeypatch):
    monkeypatch.setattr(S, "load", lambda require_gpu=False: StubLib(0))
    B, T, R = 2, 6, 3
    lt = torch.zeros((B, T, R, 2))
    bs = torch.zeros((B, T), dtype=torch.int32)
    sl = pl = torch.ones(B, dtype=torch.int32)
    with pytest.raises(ValueError):
        S.ssnt_fwd_bwd_band(torch.zeros((B, T, R)), bs, sl, pl)
    with pytest.raises(ValueError):
        S.ssnt_fwd_bwd_band(torch.zeros((B, T, R, 3)), bs, sl, pl)
    with pytest.raises(TypeError):
        S.ssnt_fwd_bwd_band(lt, bs.float(), sl, pl)
    with pytest.raises(ValueError):
        S.ssnt_fwd_bwd_band(lt, bs[:, :5], sl, pl)
    with pytest.raises(ValueError):
        S.ssnt_fwd_bwd_band(lt, bs, sl, pl, torch.zeros((B, T, R + 1)))
    with pytest.raises(ValueError):
        S.ssnt_fwd_bwd_band(lt, bs, sl, pl, out={"grad": torch.zeros((B, T, R))})
    with pytest.raises(TypeError):
        S.ssnt_fwd_bwd_band(lt, [[0] * T] * B, sl, pl)


def test_new_names_are_public():
    for name in ("ssnt_fwd_bwd_band", "SSNTBandLatticeLoss", "ssnt_band_lattice_loss",
                 "ssnt_band_from_positions", "ssnt_band_gather", "ssnt_band_scatter"):
        assert name in S.__all__ and name in S.__doc__ and hasattr(S, name)
