"""The streaming fwd-bwd kernel's row path: the converters step their load address from row to
row (no address formed from the row number) and the chain rows are planar within a lane's slice.
Both can go wrong only at particular lengths -- the residues of S around the ring size 8, the
converter block 8 and the 3-converter stride; S < T (zero fill, prefetches past the utterance's
end) and S = T (prefetches past the tensor's) -- so every case here runs all of them, bit-exact
against oracle.fwd_bwd_xf on loss, grad (grad_obs) and the debug rows.

Every tensor a stepped address reaches (log_trans, log_obs, grad, grad_obs) is a view into the
middle of a larger allocation with a whole utterance (T rows) of slack on each side: NaN on the
input side, a sentinel bit pattern on the output side. An address one row or one utterance off
therefore stays inside allocated memory: it shows as a mismatch or a damaged sentinel."""
import functools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent

S_VALUES = (1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 23, 24, 25, 26, 39, 40)
SENTINEL = 0x7FC0DEAD  # a NaN payload, read back as int32
STATUS_TIMEOUT, STATUS_RING_TAG = 1 << 4, 1 << 5  # ssnt_internal.h

# name -> (B, T, U, offset of the views in floats): the kernel instance each one reaches
INSTANCES = {
    "K2-U80": (3, 40, 80, 0),         # K = 2, vector form
    "K1-U64": (3, 40, 64, 0),         # K = 1
    "narrow-U81": (3, 40, 81, 0),     # U % K != 0: one access per position
    "narrow-U81-off4": (3, 40, 81, 1),  # ... and the views at a 4-byte offset
    "K4-U160": (3, 40, 160, 0),       # K = 4 (10 waves)
    "ws-T320-U80": (2, 320, 80, 0),   # storage rows in the workspace (LDS = 0)
}
FLAGS = {"term": 1, "noterm": 0, "term-zeroinf": 1 | 2}


def batches(B, T, U):
    """Every (S, P) with S in S_VALUES (and T) and P in {1, ceil(S/2), min(S, U)}, B utterances
    at a time with different S in one batch; one utterance with S < P (infeasible) at the end."""
    sv = sorted(set(S_VALUES) | {T})
    sv = [s for s in sv if s <= T]
    pairs = []
    for k in range(3):  # rotate P's choice against S so that a batch mixes them
        for i, s in enumerate(sv):
            pairs.append((s, (1, min((s + 1) // 2, U), min(s, U))[(i + k) % 3]))
    pairs.append((3, min(5, U)))
    out = []
    for i in range(0, len(pairs), B):
        chunk = pairs[i:i + B]
        while len(chunk) < B:  # pad the last batch with lengths not yet in it
            chunk.append(next(p for p in pairs if p[0] not in [c[0] for c in chunk]))
        assert len({c[0] for c in chunk}) == B, chunk
        out.append(([c[0] for c in chunk], [c[1] for c in chunk]))
    return out


def inputs(inst, obs):
    B, T, U, _ = INSTANCES[inst]
    import oracle as O
    lt = O.synth_log_trans(B, T, U, seed=T + U)
    lo = None
    if obs:
        rng = np.random.default_rng(U)
        lo = (-np.abs(rng.standard_normal((B, T, U), dtype=np.float32))).astype(np.float32)
    return lt, lo


@functools.lru_cache(maxsize=None)
def reference(inst, obs, flags):
    """The oracle's results for every batch of a case: computed once, shared, never modified."""
    import oracle as O
    B, T, U, _ = INSTANCES[inst]
    lt, lo = inputs(inst, obs)
    res = []
    for S, P in batches(B, T, U):
        o = O.fwd_bwd_xf(lt, S, P, log_obs=lo, flags=flags, debug=True)
        for v in o.values():
            v.setflags(write=False)
        res.append(o)
    return res


CASES = [(i, o, f) for i in INSTANCES for o in (False, True) for f in FLAGS]


@pytest.mark.parametrize("inst,obs,fl", CASES, ids=[f"{i}-{'obs' if o else 'noobs'}-{f}" for i, o, f in CASES])
def test_oracle_accepts_every_shape(oracle, inst, obs, fl):
    # CPU pre-check: the oracle alone takes every listed shape; finite loss where S >= P, the
    # infeasible result (inf, or 0 under ZERO_INFINITY) otherwise; no NaN anywhere
    B, T, U, _ = INSTANCES[inst]
    flags = FLAGS[fl]
    seen = set()
    for (S, P), o in zip(batches(B, T, U), reference(inst, obs, flags)):
        for b in range(B):
            seen.add(S[b])
            if S[b] >= P[b]:
                assert np.isfinite(o["loss"][b]), (S[b], P[b])
            else:
                assert o["loss"][b] == (0.0 if flags & 2 else np.inf), (S[b], P[b])
        assert not np.isnan(o["grad"]).any()
    assert seen >= set(S_VALUES) | {T}


class Guarded:
    """A (B, ...) float32 tensor as a view into the middle of a larger allocation, one whole
    utterance of slack on each side, `offset` floats past the allocation's alignment."""

    def __init__(self, torch, dev, shape, offset, fill):
        n = int(np.prod(shape))
        self.slack = int(np.prod(shape[1:])) + 64
        self.flat = torch.empty(2 * self.slack + n + offset, dtype=torch.float32, device=dev)
        if fill is None:
            self.flat.view(torch.int32).fill_(SENTINEL)
        else:
            self.flat.fill_(fill)
        self.lo = self.slack + offset
        self.view = self.flat[self.lo:self.lo + n].view(shape)
        self.torch = torch

    def sentinels_intact(self):
        i = self.flat.view(self.torch.int32)
        n = self.view.numel()
        return bool((i[:self.lo] == SENTINEL).all()) and bool((i[self.lo + n:] == SENTINEL).all())


def run_case(S_mod, inst, obs, flags):
    """Every batch of a case on the GPU (product instance, then the debug instance), each
    compared with the shared reference. Returns the OR of the status words."""
    import torch
    dev = torch.device("cuda:0")
    B, T, U, off = INSTANCES[inst]
    lt, lo = inputs(inst, obs)
    nan = float("nan")
    g_lt = Guarded(torch, dev, (B, T, U, 2), off, nan)
    g_lt.view.copy_(torch.from_numpy(lt))
    g_lo = None
    if obs:
        g_lo = Guarded(torch, dev, (B, T, U), off, nan)
        g_lo.view.copy_(torch.from_numpy(lo))
    bits = 0
    for (S, P), o in zip(batches(B, T, U), reference(inst, obs, flags)):
        sl = torch.tensor(S, dtype=torch.int32, device=dev)
        pl = torch.tensor(P, dtype=torch.int32, device=dev)
        for debug in (False, True):
            g_grad = Guarded(torch, dev, (B, T, U, 2), off, None)
            out = {"grad": g_grad.view}
            g_gobs = None
            if obs:
                g_gobs = Guarded(torch, dev, (B, T, U), off, None)
                out["grad_obs"] = g_gobs.view
            r = S_mod.ssnt_fwd_bwd(g_lt.view, sl, pl, g_lo.view if obs else None,
                                   terminal_emit=bool(flags & 1), zero_infinity=bool(flags & 2),
                                   debug=debug, check=False, out=out)
            torch.cuda.synchronize()
            bits |= int(r["status"].item())
            keys = ["loss", "grad"] + (["grad_obs"] if obs else []) + (["log_alpha", "log_beta"] if debug else [])
            for k in keys:
                got = r[k].cpu().numpy()
                assert got.tobytes() == o[k].tobytes(), (
                    inst, obs, flags, S, P, debug, k, S_mod.last_fwd_bwd_kernel(),
                    int((got.view(np.uint32) != o[k].view(np.uint32)).sum()))
            assert g_grad.sentinels_intact(), (inst, S, P, debug, "grad slack written")
            if obs:
                assert g_gobs.sentinels_intact(), (inst, S, P, debug, "grad_obs slack written")
    return bits


def expected_kernel(inst, obs):
    K = {"K2": 2, "K1": 1, "narrow": 2, "K4": 4, "ws": 2}[inst.split("-")[0]]
    lds = 0 if inst.startswith("ws") else 1
    nv = 1 if inst.startswith("narrow") else 0
    return f"k_fwd_bwd_stream<K={K},OBS={int(obs)},LDS={lds},", f"NV={nv}"


@pytest.mark.gpu
@pytest.mark.parametrize("inst,obs,fl", CASES, ids=[f"{i}-{'obs' if o else 'noobs'}-{f}" for i, o, f in CASES])
def test_rowpath_bit_exact_guarded(gpu, oracle, inst, obs, fl):
    bits = run_case(gpu, inst, obs, FLAGS[fl])
    assert bits == 0, bits
    head, nv = expected_kernel(inst, obs)
    k = gpu.last_fwd_bwd_kernel()
    assert k.startswith(head) and nv in k, k  # the instance this case is meant to reach


_DIAG_SCRIPT = r"""
import ctypes, sys
sys.path[:0] = sys.argv[1:4]
import ssnt_tts_amd as S
import test_gpu_stream_rowpath as R
lib = S.load()
lib.ssnt_diag_read.restype = ctypes.c_int
lib.ssnt_diag_read.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
assert lib.ssnt_diag_read(None, 0) >= 0  # a diagnostic build
for inst in ("K2-U80", "ws-T320-U80"):
    for obs in (False, True):
        bits = R.run_case(S, inst, obs, 1)
        assert not bits & (R.STATUS_TIMEOUT | R.STATUS_RING_TAG), (inst, obs, bits)
        assert bits == 0, (inst, obs, bits)
print("rowpath diag ok")
"""


@pytest.mark.gpu
def test_rowpath_diag_build_ring_tags(gpu, oracle):
    # the same cases through the diagnostic build (make lib-diag): every ring slot and chain-ring
    # row carries the row it holds, every consumer checks it; no kStatusRingTag, no kStatusTimeout
    lib = ROOT / "ssnt-tts-rust_amd" / "lib" / "diag" / "libssnt_tts_c.so"
    assert lib.exists(), "make lib-diag"
    env = dict(os.environ, SSNT_TTS_C_LIB=str(lib))
    r = subprocess.run([sys.executable, "-c", _DIAG_SCRIPT, str(ROOT / "ssnt-tts-rust_amd"),
                        str(ROOT / "oracle"), str(ROOT / "tests")], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "rowpath diag ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
