#!/usr/bin/env python3
"""Time the best-path (Viterbi) alignment against its two yardsticks, in one process on one GPU:

  ssnt_viterbi_align          B=256 T=200 U=80 and B=64 T=2000 U=400 (log_prob + position + duration)
  ssnt_fwd_bwd(need_grad)     the same two shapes (the alignment reads half its bytes, one direction)
  lattice_beam_search_decode  W=4 at the first shape (the call the alignment replaces)

GPU time as tools/bench_configs.py: HIP events around `iters` back-to-back calls, median of 5
rounds. One JSON line per shape, also written to profiles/viterbi_align.jsonl with the source
hash bench.py's roofline uses. `met` says whether the alignment took no longer than each
yardstick of the same run (no margin)."""
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
OUT = ROOT / "profiles" / "viterbi_align.jsonl"


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


def shape(B, T, U, iters, decode_w=None):
    lt = torch.from_numpy(O.synth_log_trans(B, T, U, seed=0)).to(DEV)
    sl = torch.full((B,), T, dtype=torch.int32, device=DEV)
    pl = torch.full((B,), U, dtype=torch.int32, device=DEV)
    vo = {"log_prob": torch.empty(B, device=DEV),
          "position": torch.empty((B, T), dtype=torch.int32, device=DEV),
          "duration": torch.empty((B, U), dtype=torch.int32, device=DEV),
          "status": torch.zeros(1, dtype=torch.int32, device=DEV)}
    fo = {"loss": torch.empty(B, device=DEV), "grad": torch.empty((B, T, U, 2), device=DEV),
          "status": torch.zeros(1, dtype=torch.int32, device=DEV)}
    S.ssnt_viterbi_align(lt, sl, pl, out=vo, check=True)
    S.ssnt_fwd_bwd(lt, sl, pl, out=fo, check=True)
    tv = gpu_time(lambda: S.ssnt_viterbi_align(lt, sl, pl, out=vo), iters)
    tl = gpu_time(lambda: S.ssnt_viterbi_align(lt, sl, pl, need_path=False, out={"log_prob": vo["log_prob"],
                                                                                 "status": vo["status"]}), iters)
    tf = gpu_time(lambda: S.ssnt_fwd_bwd(lt, sl, pl, need_grad=True, out=fo), iters)
    read = B * T * U * 8
    r = {"workload": f"best path B={B} T={T} U={U} (log_prob + position + duration)",
         "viterbi_us": tv * 1e6, "viterbi_log_prob_only_us": tl * 1e6, "fwd_bwd_us": tf * 1e6,
         "bytes_read": read, "hbm_frac": read / tv / 8e12,
         "workspace_bytes": int(S.load().ssnt_viterbi_align_workspace_size(B, T, U)),
         "met": {"fwd_bwd": tv <= tf}}
    if decode_w:
        il = torch.full((B,), U, dtype=torch.int32, device=DEV)
        S.lattice_beam_search_decode(lt, il, decode_w)
        td = gpu_time(lambda: S.lattice_beam_search_decode(lt, il, decode_w, check=False), iters)
        r["beam_decode_us"] = td * 1e6
        r["beam_decode_w"] = decode_w
        r["met"]["beam_decode"] = tv <= td
    r["source_sha"] = kernel_source_sha()
    r["device"] = torch.cuda.get_device_name(0)
    return r


def main():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", type=Path, default=OUT, help="JSON-lines file to (over)write")
    out = ap.parse_args().out
    rows = [shape(256, 200, 80, 200, decode_w=4), shape(64, 2000, 400, 20)]
    out.parent.mkdir(parents=True, exist_ok=True)
    with open(out, "w") as f:
        for r in rows:
            line = json.dumps(r)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
