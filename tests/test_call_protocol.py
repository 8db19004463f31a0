"""The mirror's host call protocol (ssnt_tts_amd._Call, _v2_inputs; DESIGN.md "Host call
protocol") on CPU tensors, with a stub in place of the library function: no GPU needed."""
import ctypes

import pytest
import torch

import ssnt_tts_amd as S


@pytest.fixture
def cpu(monkeypatch):
    """The helpers that insist on the GPU, relaxed: any device's tensors, no stream."""
    monkeypatch.setattr(S, "_stream", lambda dev: None)
    monkeypatch.setattr(S, "_dev", lambda t, dtype, name: t.to(dtype).contiguous())
    return torch.device("cpu")


class Stub:
    """Records what a C entry would receive; answers `rc`."""

    def __init__(self, rc=0, status=-2):
        self.rc, self.status, self.args, self.status_at_call = rc, status, None, None

    def __call__(self, *args):
        self.args = args
        self.status_at_call = ctypes.cast(args[self.status], ctypes.POINTER(ctypes.c_int))[0]
        return self.rc


def test_out_tensors_are_reused_and_unwanted_outputs_are_null(cpu):
    mine = torch.empty((2, 3), dtype=torch.int32)
    c = S._Call("stub", cpu, {"position": mine}, False)
    lp = c.buf("log_prob", (2,))
    pos = c.buf("position", (2, 3), torch.int32)
    dur = c.buf("duration", (2, 5), torch.int32, want=False)
    assert pos == mine.data_ptr() and dur is None  # (buf answers with the address)
    c.workspace(lambda *shape: sum(shape), 2, 3, 5)
    fn = Stub()
    res = c.run(fn, lp, None, 7, lp, pos, dur)
    assert set(res) == {"log_prob", "position", "status"} and res["position"] is mine
    a = fn.args
    assert len(a) == 6 + 4 and a[1] is None and a[2] == 7 and a[5] is None  # None, an int, not wanted
    assert a[0] == a[3] == lp == res["log_prob"].data_ptr() and a[4] == mine.data_ptr()
    assert a[6] == c.ws.data_ptr() and a[7] == 10 == c.ws.numel()
    assert a[8] == res["status"].data_ptr() and a[9] is None


def test_no_workspace_is_null_and_the_tail_follows_the_status(cpu):
    c = S._Call("stub", cpu, None, False)
    fn = Stub(status=-3)
    c.run(fn, tail=(torch.zeros(1).data_ptr(),))
    assert fn.args[0] is None and fn.args[1] == 0 and len(fn.args) == 5  # ws, bytes, status, tail, stream
    assert fn.args[3] is not None


@pytest.mark.parametrize("bad", [torch.empty((2, 4)), torch.empty((2, 3), dtype=torch.float64),
                                 torch.empty((3, 2)).t()], ids=["shape", "dtype", "non-contiguous"])
def test_a_wrong_out_tensor_is_refused_before_the_call(cpu, bad):
    c = S._Call("stub", cpu, {"loss": bad}, False)
    with pytest.raises(ValueError):
        c.buf("loss", (2, 3))
    assert "loss" not in c.res


def test_a_given_status_word_is_zeroed_before_the_call(cpu):
    st = torch.full((1,), 4, dtype=torch.int32)
    fn = Stub()
    res = S._Call("stub", cpu, {"status": st}, False).run(fn)
    assert fn.status_at_call == 0 and res["status"] is st
    fresh = S._Call("stub", cpu, None, False).run(fn)["status"]
    assert fn.status_at_call == 0 and fresh is not st and fresh.dtype == torch.int32
    with pytest.raises(S.SsntError):  # the entry's return code
        S._Call("stub", cpu, None, False).run(Stub(rc=6))


def test_v2_inputs_reads_the_device_only_without_max_total(cpu, monkeypatch):
    def item(self):
        raise AssertionError("device read-back")

    lg, tb = torch.zeros((2, 5, 3)), torch.arange(3)
    il, ol = torch.tensor([5, 4]), torch.tensor([9, 7])
    assert S._v2_inputs(lg, tb, il, ol, None)[4] == 9
    monkeypatch.setattr(torch.Tensor, "item", item)
    g, t, i, o, mt = S._v2_inputs(lg, tb, il, ol, 8)
    assert mt == 8 and g.dtype == torch.float32 and {t.dtype, i.dtype, o.dtype} == {torch.int32}
    assert t.shape == (3,) and i.shape == o.shape == (2,)
    with pytest.raises(AssertionError):
        S._v2_inputs(lg, tb, il, ol, None)
