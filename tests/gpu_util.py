"""What the GPU test files share (test infrastructure only): numpy to device tensor, a tensor's
address for a raw ctypes call, the search for the shape at which a size query switches from LDS
to a workspace, and the runs of a C entry over a poisoned workspace."""
import ctypes

import numpy as np
import torch

import guarded as G

DEV = "cuda:0"


def _t(x, dtype=None, dev=DEV):
    """The numpy array `x` as a contiguous tensor on `dev` (None stays None)."""
    if x is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).to(dev)


def vp(t):
    """A tensor (or an integer address) as the pointer argument of a raw ctypes call; None is NULL."""
    return None if t is None else ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr())


def switch_point(query, hi=1 << 16):
    """The largest n in [1, hi) with query(n) == 0, for a size query that is 0 up to some n and
    positive beyond it (the rows stay in LDS / go to the workspace)."""
    lo = 1
    assert query(lo) == 0 and query(hi) > 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if query(mid) == 0 else (lo, mid)
    return lo


def poisoned_runs(arena, v, put, call, x, other, keys, ws="ws"):
    """A C entry over a `guarded.lay_out` arena (arena, v) whose workspace v[ws] is filled with
    0xFF, with 0x00, and left as a finished run on the input `other` wrote it. `put(x)` writes an
    input into the arena, `call()` runs the entry and returns its status code. After every run the
    code and v["status"] are 0 and the guards intact. Returns the three results {k: v[k]} of the
    runs on `x`."""
    res = []
    for fill in (0xFF, 0x00, "stale"):
        for inp in ([x] if fill != "stale" else [other, x]):  # stale: another input's run first
            put(inp)
            if fill != "stale":
                G.fill_bytes(v[ws], fill)
            v["status"].zero_()
            assert call() == 0
            if v["status"].is_cuda:
                torch.cuda.synchronize()
            assert int(v["status"].item()) == 0
            arena.check()
        res.append({k: G.get(v[k]) for k in keys})
    return res
