"""A guarded arena for the contract tests (tests/test_gpu_contract.py): every tensor
of a call -- inputs, outputs, workspace, state -- is a view into one uint8 allocation, exactly as
long as its contract says, with a zone of a known byte immediately before and after it. A kernel
that writes a byte outside what it was given damages a zone (``check``); one that reads outside
reads the zone's byte, which the tests change between runs. Works on CPU tensors too
(tests/test_guarded.py). Test infrastructure only."""
import ctypes

import numpy as np
import torch

# one U = 1024 row of 8-byte cells, doubled: an overrun by a whole row stays inside the arena
GUARD = 16384


class Arena:
    """One uint8 tensor of `nbytes` on `device`, handed out front to back by take()."""

    def __init__(self, device, nbytes, guard=GUARD, byte=0xA5):
        self.buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        self.base = self.buf.data_ptr()
        self.guard = int(guard)
        self.byte = int(byte)
        self.blocks = []  # dicts: name, start, end (byte offsets of the view), before, after
        self.cursor = 0   # first byte no block or guard owns yet

    @staticmethod
    def room(nbytes, align=256, offset=0, guard=GUARD):
        """An upper bound on what one take() of `nbytes` consumes."""
        return int(nbytes) + 2 * guard + align + offset

    def take(self, shape, dtype, align=256, offset=0, name=None):
        """A view of exactly numel * itemsize bytes whose address is `offset` bytes past a multiple
        of `align`. The guard before it runs from the previous block's guard (the alignment slack
        belongs to it: at least `guard` bytes); the guard after it starts at the view's last byte
        + 1, with no rounding."""
        shape = (int(shape),) if isinstance(shape, (int, np.integer)) else tuple(int(x) for x in shape)
        item = torch.empty((), dtype=dtype).element_size()
        assert 0 <= offset < align and offset % item == 0 and self.base % item == 0
        nbytes = int(np.prod(shape, dtype=np.int64)) * item
        addr = self.base + self.cursor + self.guard
        addr += (offset - addr) % align
        start = addr - self.base
        end = start + nbytes
        if end + self.guard > self.buf.numel():
            raise ValueError(f"arena of {self.buf.numel()} bytes is full at block {len(self.blocks)}")
        blk = {"name": name or f"block{len(self.blocks)}", "start": start, "end": end,
               "before": (self.cursor, start), "after": (end, end + self.guard)}
        self.blocks.append(blk)
        self.cursor = end + self.guard
        for lo, hi in (blk["before"], blk["after"]):
            self.buf[lo:hi] = self.byte
        return self.buf[start:end].view(dtype).view(shape)

    def fill_guards(self, byte):
        """Refill every guard with `byte` (what check() then expects)."""
        self.byte = int(byte)
        for blk in self.blocks:
            for lo, hi in (blk["before"], blk["after"]):
                self.buf[lo:hi] = self.byte

    def check(self):
        """Assert every guard intact; name the block, the side and the first damaged offset
        (before: bytes back from the block's first byte; after: bytes past its last byte)."""
        zones = [(blk, side) + blk[side] for blk in self.blocks for side in ("before", "after")]
        if not zones:
            return
        bad = torch.stack([torch.count_nonzero(self.buf[lo:hi] != self.byte) for _, _, lo, hi in zones])
        if int(bad.sum()) == 0:
            return
        for (blk, side, lo, hi), n in zip(zones, bad.tolist()):
            if n == 0:
                continue
            at = lo + int(torch.nonzero(self.buf[lo:hi] != self.byte)[0])
            if side == "before":
                where = f"{blk['start'] - at} bytes before its first byte"
            else:
                where = f"{at - blk['end'] + 1} bytes after its last byte"
            raise AssertionError(f"guard {side} block {blk['name']!r} damaged: {n} bytes, the first "
                                 f"{where} (arena offset {at}, value {int(self.buf[at]):#04x}, "
                                 f"guard byte {self.byte:#04x})")


def lay_out(device, specs, byte=0xA5):
    """specs: name -> (shape, dtype) or (shape, dtype, offset). One arena sized for them and the
    dict of views, in the order given."""
    norm = {k: (v if len(v) == 3 else (*v, 0)) for k, v in specs.items()}
    need = 0
    for shape, dtype, off in norm.values():
        n = int(np.prod(np.atleast_1d(shape), dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
        need += Arena.room(n, offset=off)
    arena = Arena(device, need, byte=byte)
    return arena, {k: arena.take(shape, dtype, offset=off, name=k) for k, (shape, dtype, off) in norm.items()}


def fill_bytes(t, byte):
    """Every byte of the contiguous tensor `t` := byte."""
    if t is not None and t.numel():
        t.view(-1).view(torch.uint8).fill_(int(byte))


def put(t, a):
    """Copy the numpy array `a` into the view `t` bit for bit (NaN payloads included)."""
    a = np.ascontiguousarray(a)
    assert tuple(a.shape) == tuple(t.shape), (a.shape, t.shape)
    if a.size:
        t.view(-1).view(torch.uint8).copy_(torch.from_numpy(a.reshape(-1).view(np.uint8)))


def get(t):
    """The view `t` as a numpy array (a copy)."""
    return t.detach().cpu().numpy().copy()


def call(lib, name, *args):
    """lib.<name>(*args) with the argument order of ssnt_tts_amd._lib.SIGNATURES: a tensor goes in
    as the address of its first byte, None as NULL, and only where the signature has a pointer."""
    from ssnt_tts_amd._lib import AB_SIGNATURES, SIGNATURES
    _, argtypes = {**AB_SIGNATURES, **SIGNATURES}[name]
    assert len(args) == len(argtypes), (name, len(args), len(argtypes))
    conv = []
    for i, (a, ty) in enumerate(zip(args, argtypes)):
        if isinstance(a, torch.Tensor):
            assert ty is ctypes.c_void_p and a.is_contiguous(), (name, i)
            a = ctypes.c_void_p(a.data_ptr())
        elif ty is ctypes.c_void_p:
            assert a is None or isinstance(a, (int, ctypes.c_void_p)), (name, i, type(a))
            a = ctypes.c_void_p(a) if isinstance(a, int) else a
        else:
            assert a is not None and not isinstance(a, ctypes.c_void_p), (name, i)
        conv.append(a)
    return getattr(lib, name)(*conv)
