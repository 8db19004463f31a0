#!/usr/bin/env python3
"""Time the best duration path on the v2 lattice against its two yardsticks, in one process on
one GPU, at the configs[4] shape (B=64 I=400 O=2000 D=16), band mode and test mode:

  v2_viterbi_align                  log_prob + duration_class + duration + total
  v2_fwd_bwd(need_grad=False)       the sum over the same lattice (two sweeps, split-exponent)
  v2_lattice_beam_search_decode     W=4, the pruned search the exact path replaces

GPU time as tools/bench_viterbi.py: HIP events around `iters` back-to-back calls, median of 5
rounds. One JSON line per mode, also written to profiles/v2_viterbi.jsonl with the source hash
bench.py's roofline uses. `met` says whether the alignment took no longer than each yardstick of
the same run (no margin); `viterbi_log_prob_only_us` (no backpointers, no backtrace) splits the
alignment's time into sweep and path."""
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

DEV = torch.device("cuda:0")
OUT = ROOT / "profiles" / "v2_viterbi.jsonl"


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


def mode(test_mode, iters, B=64, I=400, Ot=2000, D=16, W=4):
    d = O.synth_durations(B, I, Ot, D, seed=0)
    lg = torch.from_numpy(O.synth_v2_step_logits(d, D, seed=1)).to(DEV)
    lg4 = lg[:, :, None, :].expand(-1, -1, W, -1).contiguous()
    table = torch.arange(D, dtype=torch.int32, device=DEV)
    il = torch.full((B,), I, dtype=torch.int32, device=DEV)
    ol = torch.full((B,), Ot, dtype=torch.int32, device=DEV)
    kw = dict(allow_skip=False, test_mode=test_mode, max_total=Ot)
    vo = {"log_prob": torch.empty(B, device=DEV),
          "duration_class": torch.empty((B, I), dtype=torch.int32, device=DEV),
          "duration": torch.empty((B, I), dtype=torch.int32, device=DEV),
          "total": torch.empty(B, dtype=torch.int32, device=DEV),
          "status": torch.zeros(1, dtype=torch.int32, device=DEV)}
    lo = {"log_prob": vo["log_prob"], "status": vo["status"]}
    S.v2_viterbi_align(lg, table, il, ol, 0, out=vo, check=True, **kw)
    S.v2_fwd_bwd(lg, table, il, ol, 0, need_grad=False, check=True, **kw)
    tv = gpu_time(lambda: S.v2_viterbi_align(lg, table, il, ol, 0, out=vo, **kw), iters)
    tl = gpu_time(lambda: S.v2_viterbi_align(lg, table, il, ol, 0, need_path=False, out=lo, **kw), iters)
    tf = gpu_time(lambda: S.v2_fwd_bwd(lg, table, il, ol, 0, need_grad=False, **kw), iters)
    td = gpu_time(lambda: S.v2_lattice_beam_search_decode(lg4, table, il, ol, W, 0, False, test_mode,
                                                          check=False), iters)
    return {"workload": f"v2 best path B={B} I={I} O={Ot} D={D} {'test' if test_mode else 'band'} mode "
                        "(log_prob + duration_class + duration + total)",
            "test_mode": bool(test_mode),
            "viterbi_us": tv * 1e6, "viterbi_log_prob_only_us": tl * 1e6,
            "fwd_bwd_no_grad_us": tf * 1e6, "beam_decode_us": td * 1e6, "beam_decode_w": W,
            "ratio_to_fwd_bwd": tv / tf, "ratio_to_beam_decode": tv / td,
            "workspace_bytes": int(S.load().ssnt_v2_viterbi_align_workspace_size(B, I, Ot, test_mode)),
            "met": {"fwd_bwd": tv <= tf, "beam_decode": tv <= td},
            "source_sha": kernel_source_sha(), "device": torch.cuda.get_device_name(0)}


def main():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", type=Path, default=OUT, help="JSON-lines file to (over)write")
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    rows = [mode(False, a.iters), mode(True, a.iters)]
    a.out.parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            line = json.dumps(r)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
