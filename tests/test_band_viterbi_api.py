"""The banded best path's host layer without a GPU: ssnt_band_edge_contact on hand-made cases, the
two new symbols in header, library and ctypes table, the wrapper's argument order with a stub in
place of the library, and its loud failure without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import ssnt_tts_amd as S
from test_capi_exports import LIB, _exported, header_functions

NEW = ("ssnt_viterbi_align_band_workspace_size", "ssnt_viterbi_align_band_device")


def test_edge_contact_on_hand_made_cases():
    R = 3
    #                 s:  0  1  2  3  4  5  6  7
    bs = torch.tensor([[0, 0, 1, 1, 2, 2, 2, 2],    # P = 6: lattice beyond the right edge until bs + R = 6
                       [0, 0, 0, 1, 1, 1, 1, 1],    # P = 4: the right edge is the lattice's own from s = 3
                       [0, 1, 2, 3, 3, 3, 3, 3],    # the path on the left edge of a moving band
                       [0, 0, 0, 0, 0, 0, 0, 0],    # infeasible
                       [0, 0, 1, 1, 1, 9, 9, 9]],   # S = 5: steps beyond S are not counted
                      dtype=torch.int32)
    pos = torch.tensor([[0, 1, 2, 3, 4, 4, 5, 5],   # r = 0 1 1 2 2 2 3x -> see below
                        [0, 1, 2, 2, 3, 3, 3, 3],
                        [0, 1, 2, 3, 4, 5, 5, 5],
                        [-1] * 8,
                        [0, 0, 1, 2, 3, 9, 9, 9]], dtype=torch.int32)
    pos[0, 6:] = 4                                   # r = 2 at s = 6, 7 with bs + R = 5 < 6
    sl = torch.tensor([8, 8, 8, 8, 5])
    pl = torch.tensor([6, 4, 6, 4, 5])
    got = S.ssnt_band_edge_contact(pos, bs, sl, pl, R)
    assert got.dtype == torch.int32 and tuple(got.shape) == (5,)
    # 0: r = 2 at s = 3 (bs 1: 4 < 6), s = 4, 5, 6, 7 (bs 2: 5 < 6) -> 5; r = 0 only at s = 0, bs = 0
    # 1: r = 2 at s = 2 (bs 0: 3 < 4) counts; at s = 4.. (bs 1: 4 = P) it does not -> 1
    # 2: r = 0 with bs > 0 at s = 1, 2, 3 -> 3; r = 2 at s = 5.. with bs + R = 6 = P does not count
    # 4: r = 2 at s = 4 (bs 1: 4 < 5) -> 1; r = 0 with bs > 0 at s = 2 -> 1
    want = np.zeros(5, np.int64)
    for b in range(5):
        for s in range(int(sl[b])):
            p, st = int(pos[b, s]), int(bs[b, s])
            if p < 0:
                continue
            r = p - st
            want[b] += (r == 0 and st > 0) or (r == R - 1 and st + R < int(pl[b]))
    assert want.tolist() == [5, 1, 3, 0, 2]
    assert got.tolist() == want.tolist()
    # int64 inputs and list lengths give the same
    again = S.ssnt_band_edge_contact(pos.long(), bs.long(), sl.tolist(), pl.tolist(), R)
    assert torch.equal(again, got)
    # width 1: both edges are the same column (s = 0: lattice to the right; s = 1, 2: to the left)
    one = S.ssnt_band_edge_contact(torch.tensor([[0, 1, 2]]), torch.tensor([[0, 1, 2]]), [3], [3], 1)
    assert one.tolist() == [3]
    with pytest.raises(TypeError):
        S.ssnt_band_edge_contact(pos.float(), bs, sl, pl, R)
    with pytest.raises(ValueError):
        S.ssnt_band_edge_contact(pos, bs[:, :4], sl, pl, R)
    with pytest.raises(ValueError):
        S.ssnt_band_edge_contact(pos, bs, sl, pl, 0)


def test_header_library_and_table_have_the_new_symbols():
    from ssnt_tts_amd._lib import SIGNATURES, load
    fns = header_functions()
    exported = _exported(LIB)
    for name in NEW:
        assert name in fns and name in exported and name in SIGNATURES
    assert len(SIGNATURES[NEW[1]][1]) == 17
    lib = load()  # dlopen only
    q = lib.ssnt_viterbi_align_band_workspace_size
    # host-only query: 0 in LDS mode and for refused shapes, else 8 bytes per step and 64 columns
    assert q(2, 100, 8) == 0 and q(2, 100, 0) == 0 and q(2, 100, 257) == 0 and q(0, 100, 8) == 0
    assert q(2, 12000, 8) == 2 * 12000 * 8 and q(3, 12000, 130) == 3 * 12000 * 4 * 8
    assert q(2, 1 << 20, 8) == 0  # (refused: the staged band_start does not fit)


class StubLib:
    def __init__(self, ws_bytes):
        self.ws_bytes, self.query, self.args, self.status_at_call = ws_bytes, None, None, None

    def ssnt_viterbi_align_band_workspace_size(self, *shape):
        self.query = shape
        return self.ws_bytes

    def ssnt_viterbi_align_band_device(self, *args):
        self.args = args
        self.status_at_call = ctypes.cast(args[15], ctypes.POINTER(ctypes.c_int))[0]
        return 0

    def ssnt_status_from_bits(self, bits):
        return 0


@pytest.fixture
def cpu(monkeypatch):
    monkeypatch.setattr(S, "_stream", lambda dev: None)
    monkeypatch.setattr(S, "_dev", lambda t, dtype, name: t.to(dtype).contiguous())
    return torch.device("cpu")


def test_wrapper_argument_order(cpu, monkeypatch):
    B, T, R = 2, 6, 3
    lt, lo = torch.zeros((B, T, R, 2)), torch.zeros((B, T, R))
    bs = torch.zeros((B, T), dtype=torch.int64)
    sl, pl = torch.tensor([6, 5], dtype=torch.int32), torch.tensor([2, 3], dtype=torch.int32)
    stub = StubLib(48)
    monkeypatch.setattr(S, "load", lambda require_gpu=False: stub)
    mine = torch.empty((B,))
    r = S.ssnt_viterbi_align_band(lt, bs, sl, pl, lo, max_pos=4, out={"log_prob": mine})
    a = stub.args
    assert len(a) == 17 and stub.query == (B, T, R)
    assert a[0] == lt.data_ptr() and a[1] == lo.data_ptr() and a[3] == sl.data_ptr() and a[4] == pl.data_ptr()
    assert a[2] not in (None, bs.data_ptr())  # converted to i32
    assert a[5:10] == (B, T, R, 4, S.FLAG_TERMINAL_EMIT)
    assert a[10] == mine.data_ptr() and r["log_prob"] is mine
    assert a[11] == r["position"].data_ptr() and tuple(r["position"].shape) == (B, T)
    assert a[12] == r["duration"].data_ptr() and tuple(r["duration"].shape) == (B, 4)
    assert r["position"].dtype == r["duration"].dtype == torch.int32
    assert a[13] is not None and a[14] == 48
    assert a[15] == r["status"].data_ptr() and stub.status_at_call == 0 and a[16] is None
    # no max_pos: no duration; no path: no workspace query, NULL outputs
    r = S.ssnt_viterbi_align_band(lt, bs, sl, pl, terminal_emit=False)
    assert set(r) == {"log_prob", "position", "status"} and stub.args[12] is None and stub.args[9] == 0
    assert stub.args[1] is None
    stub2 = StubLib(48)
    monkeypatch.setattr(S, "load", lambda require_gpu=False: stub2)
    r = S.ssnt_viterbi_align_band(lt, bs, sl, pl, need_path=False, max_pos=4)
    a = stub2.args
    assert stub2.query is None and a[11] is None and a[12] is None and a[13] is None and a[14] == 0
    assert set(r) == {"log_prob", "status"}
    for bad in (dict(log_trans_band=torch.zeros((B, T, R))), dict(band_start=bs.float()),
                dict(band_start=bs[:, :5]), dict(log_obs_band=torch.zeros((B, T, R + 1))), dict(max_pos=-1)):
        kw = dict(log_trans_band=lt, band_start=bs, step_len=sl, pos_len=pl)
        kw.update(bad)
        with pytest.raises((ValueError, TypeError)):
            S.ssnt_viterbi_align_band(**kw)


def test_new_names_are_public():
    for name in ("ssnt_viterbi_align_band", "ssnt_band_edge_contact"):
        assert name in S.__all__ and name in S.__doc__ and hasattr(S, name)


def test_wrapper_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError):
        S.ssnt_viterbi_align_band(torch.zeros(1, 2, 2, 2), torch.zeros((1, 2), dtype=torch.int32),
                                  torch.ones(1), torch.ones(1))
