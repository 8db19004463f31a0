#!/usr/bin/env python3
"""Time the exact N best duration paths on the v2 lattice against their yardsticks, in one process
on one GPU, at the configs[4] shape (B=64 I=400 O=2000 D=16): band mode N = 1, 2, 4, 8, test mode
N = 1, 2, 4.

  v2_nbest_align                    with paths and log_prob only, through the Python mirror and
                                    through the C entry alone (preallocated outputs and workspace),
                                    on the peaked configs[4] logits and on flat random ones
  v2_viterbi_align                  the same forms; its C entry is measured twice, before and after
                                    the N-best runs of its mode: their difference is the spread
  v2_fwd_bwd(need_grad=False)       the sum over the same lattice
  v2_lattice_beam_search_decode     W = N, the pruned search the exact list replaces

GPU time as tools/bench_v2_viterbi.py: HIP events around `iters` back-to-back calls, median of 5
rounds. One JSON line per (mode, N), also written to profiles/v2_nbest_align.jsonl with the source
hash bench.py's roofline uses. `n1_expectation` (N = 1 rows): whether N = 1 by the C entry costs
what v2_viterbi_align by its C entry costs, the margin being the spread of the latter's two
measurements. --no-skip-lib names a build of the library with -DSSNT_V2NB_SKIP=0 (the merge without
its wave-uniform shortcut) under a soname of its own, so that it loads beside the product: its C
entry is timed on the same inputs and its outputs are compared bit for bit."""
import ctypes
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "oracle", ROOT / "ssnt-tts-rust_amd"):
    sys.path.insert(0, str(p))
import oracle as O  # noqa: E402
import ssnt_tts_amd as S  # noqa: E402
from bench import kernel_source_sha  # noqa: E402
from ssnt_tts_amd._lib import SIGNATURES  # noqa: E402

DEV = torch.device("cuda:0")
OUT = ROOT / "profiles" / "v2_nbest_align.jsonl"


def gpu_time(fn, iters, rounds=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / iters * 1e-3)
    return float(np.median(ts))


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _bind(lib, name):
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = SIGNATURES[name]
    return fn


class Shape:
    def __init__(self, test_mode, B=64, I=400, Ot=2000, D=16):
        self.B, self.I, self.Ot, self.D, self.test_mode = B, I, Ot, D, bool(test_mode)
        d = O.synth_durations(B, I, Ot, D, seed=0)
        self.peaked = torch.from_numpy(O.synth_v2_step_logits(d, D, seed=1)).to(DEV)
        z = torch.from_numpy(np.random.default_rng(7).standard_normal((B, I, D)).astype(np.float32) * 1.5)
        self.flat = torch.log_softmax(z, -1).to(DEV)
        self.table = torch.arange(D, dtype=torch.int32, device=DEV)
        self.il = torch.full((B,), I, dtype=torch.int32, device=DEV)
        self.ol = torch.full((B,), Ot, dtype=torch.int32, device=DEV)
        self.kw = dict(allow_skip=False, test_mode=self.test_mode, max_total=Ot)
        self.status = torch.zeros(1, dtype=torch.int32, device=DEV)

    def outs(self, N=None):
        n = () if N is None else (N,)
        B, I = self.B, self.I
        return {"log_prob": torch.empty((B, *n), device=DEV),
                "duration_class": torch.empty((B, *n, I), dtype=torch.int32, device=DEV),
                "duration": torch.empty((B, *n, I), dtype=torch.int32, device=DEV),
                "total": torch.empty((B, *n), dtype=torch.int32, device=DEV), "status": self.status}

    def c_viterbi(self, lib, o, path=True):
        """v2_viterbi_align through its C entry alone."""
        fn = _bind(lib, "ssnt_v2_viterbi_align_device")
        need = int(_bind(lib, "ssnt_v2_viterbi_align_workspace_size")(self.B, self.I, self.Ot, self.test_mode))
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=DEV)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        a = (_vp(self.peaked), _vp(self.table), _vp(self.il), _vp(self.ol), self.B, self.I, self.D, self.Ot, 0,
             False, self.test_mode, _vp(o["log_prob"]), _vp(o["duration_class"]) if path else None,
             _vp(o["duration"]) if path else None, _vp(o["total"]), _vp(ws), need, _vp(self.status), st)
        return lambda: fn(*a)

    def c_nbest(self, lib, lg, N, o, path=True):
        """v2_nbest_align through its C entry alone; returns the call and the workspace bytes."""
        fn = _bind(lib, "ssnt_v2_nbest_align_device")
        need = int(_bind(lib, "ssnt_v2_nbest_align_workspace_size")(self.B, self.I, self.Ot, self.test_mode, N))
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=DEV)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        a = (_vp(lg), _vp(self.table), _vp(self.il), _vp(self.ol), self.B, self.I, self.D, self.Ot, 0, False,
             self.test_mode, N, _vp(o["log_prob"]), _vp(o["duration_class"]) if path else None,
             _vp(o["duration"]) if path else None, _vp(o["total"]), _vp(ws), need, _vp(self.status), st)

        def call():
            rc = fn(*a)
            assert rc == 0, rc
        return call, need


def mode(test_mode, Ns, iters, noskip):
    s = Shape(test_mode)
    lib = S.load()
    us = lambda t: t * 1e6  # noqa: E731
    vo = s.outs()
    vargs = (s.peaked, s.table, s.il, s.ol, 0)
    S.v2_viterbi_align(*vargs, out=vo, check=True, **s.kw)
    S.v2_fwd_bwd(*vargs, need_grad=False, check=True, **s.kw)
    vit = {"mirror_us": us(gpu_time(lambda: S.v2_viterbi_align(*vargs, out=vo, **s.kw), iters)),
           "mirror_log_prob_only_us": us(gpu_time(lambda: S.v2_viterbi_align(
               *vargs, need_path=False, out={"log_prob": vo["log_prob"], "status": s.status}, **s.kw), iters)),
           "c_entry_us_first": us(gpu_time(s.c_viterbi(lib, vo), iters)),
           "c_entry_log_prob_only_us": us(gpu_time(s.c_viterbi(lib, vo, False), iters))}
    fwd = us(gpu_time(lambda: S.v2_fwd_bwd(*vargs, need_grad=False, **s.kw), iters))
    rows = []
    for N in Ns:
        o = s.outs(N)
        r = S.v2_nbest_align(*vargs, N, out=o, check=True, **s.kw)
        assert bool(torch.all(r["count"] == N))
        want = {k: o[k].clone() for k in ("log_prob", "duration_class", "duration", "total")}
        lo = {"log_prob": o["log_prob"], "status": s.status}
        c_path, need = s.c_nbest(lib, s.peaked, N, o)
        c_lp, _ = s.c_nbest(lib, s.peaked, N, o, False)
        c_flat, _ = s.c_nbest(lib, s.flat, N, o)
        row = {"workload": f"v2 N-best paths B={s.B} I={s.I} O={s.Ot} D={s.D} "
                           f"{'test' if test_mode else 'band'} mode N={N}",
               "test_mode": bool(test_mode), "num_best": N, "workspace_bytes": need,
               "mirror_us": us(gpu_time(lambda: S.v2_nbest_align(*vargs, N, out=o, **s.kw), iters)),
               "mirror_log_prob_only_us": us(gpu_time(
                   lambda: S.v2_nbest_align(*vargs, N, need_path=False, out=lo, **s.kw), iters)),
               "c_entry_us": us(gpu_time(c_path, iters)),
               "c_entry_log_prob_only_us": us(gpu_time(c_lp, iters)),
               "c_entry_flat_logits_us": us(gpu_time(c_flat, iters))}
        if noskip is not None:  # the merge without its shortcut: same bits, its own time
            flat_want = {k: o[k].clone() for k in want}
            n_path, _ = s.c_nbest(noskip, s.peaked, N, o)
            n_flat, _ = s.c_nbest(noskip, s.flat, N, o)
            row["no_shortcut_c_entry_flat_logits_us"] = us(gpu_time(n_flat, iters))
            torch.cuda.synchronize()
            assert all(torch.equal(o[k], flat_want[k]) for k in want)
            row["no_shortcut_c_entry_us"] = us(gpu_time(n_path, iters))
            torch.cuda.synchronize()
            assert all(torch.equal(o[k], want[k]) for k in want)
        lgw = s.peaked[:, :, None, :].expand(-1, -1, N, -1).contiguous()
        row["beam_decode_us"] = us(gpu_time(lambda: S.v2_lattice_beam_search_decode(
            lgw, s.table, s.il, s.ol, N, 0, False, test_mode, check=False), iters))
        row["beam_decode_w"] = N
        rows.append(row)
    vit["c_entry_us_second"] = us(gpu_time(s.c_viterbi(lib, vo), iters))
    a, b = vit["c_entry_us_first"], vit["c_entry_us_second"]
    for row in rows:
        row.update({"viterbi": vit, "fwd_bwd_no_grad_us": fwd,
                    "ratio_to_viterbi_c_entry": row["c_entry_us"] / (0.5 * (a + b)),
                    "ratio_to_fwd_bwd": row["mirror_us"] / fwd,
                    "ratio_to_beam_decode": row["mirror_us"] / row["beam_decode_us"],
                    "source_sha": kernel_source_sha(), "device": torch.cuda.get_device_name(0)})
        if row["num_best"] == 1:
            row["n1_expectation"] = {"viterbi_spread_us": abs(a - b),
                                     "excess_us": row["c_entry_us"] - 0.5 * (a + b),
                                     "met": bool(row["c_entry_us"] - 0.5 * (a + b) <= abs(a - b))}
    return rows


def main():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", type=Path, default=OUT, help="JSON-lines file to (over)write")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-skip-lib", type=Path, default=None,
                    help="a libssnt_tts_c.so built with -DSSNT_V2NB_SKIP=0")
    a = ap.parse_args()
    noskip = ctypes.CDLL(str(a.no_skip_lib)) if a.no_skip_lib else None
    rows = mode(False, (1, 2, 4, 8), a.iters, noskip) + mode(True, (1, 2, 4), a.iters, noskip)
    a.out.parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            line = json.dumps(r)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
