"""CPU self-test of the guarded arena (tests/guarded.py): a flipped byte next to any block is
caught and attributed to that block and side; alignments and offsets are honoured; blocks and
guards tile the arena without overlap and without a gap after a block."""
import ctypes

import numpy as np
import pytest
import torch

import guarded as G

SPECS = [  # (shape, dtype, align, offset)
    ((3, 5, 7, 2), torch.float32, 256, 0),
    ((17,), torch.int32, 256, 4),       # one float past a 256-byte boundary
    ((1,), torch.uint8, 256, 0),        # one byte: the guard starts at the next byte
    ((2, 33), torch.float64, 512, 8),
    ((1001,), torch.uint8, 64, 3),      # an odd byte count
    ((0,), torch.float32, 256, 0),      # an empty block still owns its two guards
    ((5, 3), torch.float32, 16, 12),
]


def _arena(byte=0xA5):
    a = G.Arena("cpu", sum(G.Arena.room(4096, al, off) for _, _, al, off in SPECS), byte=byte)
    views = [a.take(s, d, align=al, offset=off, name=f"b{i}") for i, (s, d, al, off) in enumerate(SPECS)]
    return a, views


def test_views_have_the_requested_shape_size_alignment_and_offset():
    a, views = _arena()
    for v, blk, (shape, dtype, align, off) in zip(views, a.blocks, SPECS):
        assert tuple(v.shape) == shape and v.dtype == dtype and v.is_contiguous()
        assert blk["end"] - blk["start"] == v.numel() * v.element_size()
        assert (a.base + blk["start"]) % align == off
        if v.numel():
            assert v.data_ptr() == a.base + blk["start"]
    a.check()


def test_blocks_and_guards_tile_the_arena():
    a, _ = _arena()
    owner = np.zeros(a.buf.numel(), np.int32)
    at = 0
    for blk in a.blocks:
        (b0, b1), (a0, a1) = blk["before"], blk["after"]
        assert b0 == at, "nothing unowned between one block's guard and the next one's"
        assert b1 == blk["start"] and a0 == blk["end"], "a guard touches the block on either side"
        assert b1 - b0 >= G.GUARD and a1 - a0 == G.GUARD
        for lo, hi in ((b0, b1), (blk["start"], blk["end"]), (a0, a1)):
            owner[lo:hi] += 1
        at = a1
    assert at == a.cursor <= a.buf.numel()
    assert np.all(owner[:at] == 1) and not owner[at:].any()


def test_writes_inside_the_blocks_leave_the_guards_alone():
    a, views = _arena()
    for v in views:
        G.fill_bytes(v, 0x3C)
    a.check()
    for blk in a.blocks:
        assert bool(torch.all(a.buf[blk["start"]:blk["end"]] == 0x3C))
    for byte in (0xFF, 0x00, 0xA5):
        a.fill_guards(byte)
        a.check()
        for blk in a.blocks:
            assert bool(torch.all(a.buf[blk["start"]:blk["end"]] == 0x3C)), "fill_guards spares the blocks"
            for lo, hi in (blk["before"], blk["after"]):
                assert bool(torch.all(a.buf[lo:hi] == byte))


@pytest.mark.parametrize("byte", [0xA5, 0xFF, 0x00])
@pytest.mark.parametrize("i", range(len(SPECS)))
def test_one_flipped_byte_is_caught_and_attributed(i, byte):
    a, _ = _arena(byte)
    blk = a.blocks[i]
    cases = [(blk["start"] - 1, "before", "1 bytes before"), (blk["end"], "after", "1 bytes after"),
             (blk["before"][0], "before", f"{blk['start'] - blk['before'][0]} bytes before"),
             (blk["after"][1] - 1, "after", f"{G.GUARD} bytes after")]
    for at, side, where in cases:
        old = int(a.buf[at])
        a.buf[at] = old ^ 0x01
        with pytest.raises(AssertionError) as e:
            a.check()
        msg = str(e.value)
        assert f"guard {side} block 'b{i}'" in msg and where in msg, msg
        a.buf[at] = old
        a.check()


def test_the_first_damaged_byte_is_the_one_reported():
    a, _ = _arena()
    blk = a.blocks[2]
    a.buf[blk["end"] + 7:blk["end"] + 20] = 0
    with pytest.raises(AssertionError) as e:
        a.check()
    assert "13 bytes, the first 8 bytes after" in str(e.value), str(e.value)


def test_a_full_arena_refuses_and_lay_out_fits():
    a = G.Arena("cpu", 2 * G.GUARD + 99)
    with pytest.raises(ValueError):
        a.take((100,), torch.uint8)
    arena, v = G.lay_out("cpu", {"x": ((4, 3), torch.float32, 4), "n": ((4,), torch.int32),
                                 "ws": ((777,), torch.uint8)})
    assert [b["name"] for b in arena.blocks] == ["x", "n", "ws"]
    assert v["x"].data_ptr() % 256 == 4 and v["ws"].numel() == 777
    arena.check()


def test_put_and_get_keep_every_bit():
    _, v = G.lay_out("cpu", {"x": ((2, 3), torch.float32)})
    bits = np.array([[0x7FC00000, 0xFFFFFFFF, 0x7F800000], [0x7149F2CA, 0x42B00000, 0x80000000]], np.uint32)
    G.put(v["x"], bits.view(np.float32))
    assert np.array_equal(G.get(v["x"]).view(np.uint32), bits)


def test_call_follows_the_signature_table():
    class Lib:  # records what a C entry would receive
        def ssnt_fwd_bwd_workspace_size(self, *a):
            return a

        def ssnt_viterbi_align_device(self, *a):
            return a

    _, v = G.lay_out("cpu", {"x": ((1, 2, 2, 2), torch.float32, 4), "n": ((1,), torch.int32)})
    assert G.call(Lib(), "ssnt_fwd_bwd_workspace_size", 1, 2, 3) == (1, 2, 3)
    got = G.call(Lib(), "ssnt_viterbi_align_device", v["x"], None, v["n"], v["n"], 1, 2, 2, 1, v["x"],
                 None, None, None, 0, None, None)
    assert isinstance(got[0], ctypes.c_void_p) and got[0].value == v["x"].data_ptr()
    assert got[1] is None and got[2].value == v["n"].data_ptr() and got[4:8] == (1, 2, 2, 1)
    with pytest.raises(AssertionError):  # an argument short
        G.call(Lib(), "ssnt_fwd_bwd_workspace_size", 1, 2)
    with pytest.raises(AssertionError):  # a tensor where the signature has an int
        G.call(Lib(), "ssnt_fwd_bwd_workspace_size", v["n"], 2, 3)
    with pytest.raises(AssertionError):  # None where the signature has an int
        G.call(Lib(), "ssnt_viterbi_align_device", v["x"], None, v["n"], v["n"], None, 2, 2, 1, v["x"],
               None, None, None, 0, None, None)


# ---- gpu_util.poisoned_runs over stub entries: what the GPU tests rely on it to catch ----------
def _stub_runs(entry):
    """poisoned_runs of `entry(arena, v)` over an arena with an input, an output, a status word and a
    workspace; x and `other` differ."""
    from gpu_util import poisoned_runs
    arena, v = G.lay_out("cpu", {"x": ((8,), torch.float32), "y": ((8,), torch.float32),
                                 "status": ((1,), torch.int32), "ws": ((64,), torch.uint8)})
    x = np.arange(8, dtype=np.float32)
    return poisoned_runs(arena, v, lambda a: G.put(v["x"], a), lambda: entry(arena, v) or 0, x, x[::-1].copy(),
                         ("y",))


def test_poisoned_runs_of_a_pure_entry_agree():
    def pure(arena, v):  # writes its workspace before reading it
        v["ws"][:32].view(torch.float32).copy_(v["x"] * 2)
        v["y"].copy_(v["ws"][:32].view(torch.float32) + 1)

    res = _stub_runs(pure)
    assert len(res) == 3 and np.array_equal(res[0]["y"], np.arange(8, dtype=np.float32) * 2 + 1)
    assert all(r["y"].tobytes() == res[0]["y"].tobytes() for r in res[1:])


def test_poisoned_runs_show_a_workspace_byte_read_before_written():
    def leaky(arena, v):  # byte 40 of the workspace reaches the output unwritten
        v["y"].copy_(v["x"])
        v["y"][0] = float(v["ws"][40])
        v["ws"][40] = int(v["x"][0]) + 1

    res = _stub_runs(leaky)
    assert [float(r["y"][0]) for r in res] == [255.0, 0.0, 8.0]  # the fill, the fill, the other input's run
    assert len({r["y"].tobytes() for r in res}) == 3


def test_poisoned_runs_catch_a_write_past_the_workspace():
    def overrun(arena, v):  # one byte past the workspace's last byte
        v["y"].copy_(v["x"])
        blk = next(b for b in arena.blocks if b["name"] == "ws")
        arena.buf[blk["end"]] = 0x11

    with pytest.raises(AssertionError) as e:
        _stub_runs(overrun)
    assert "guard after block 'ws'" in str(e.value) and "1 bytes after" in str(e.value), str(e.value)
