#!/usr/bin/env python3
"""Time posterior sampling on the emit/shift lattice against its yardsticks, in one process on one GPU:

  ssnt_sample_align        B=256 T=200 U=80 with K = 1, 4, 16 and B=64 T=2000 U=400 with K = 1, 4
                           (log_prob + position + duration per sample, `uniform` given)
  ssnt_fwd_bwd(need_grad)  the same shapes (two sweeps and the gradient; the sampler does one sweep)
  ssnt_viterbi_align       the same shapes (the same sweep structure with cheaper arithmetic)

GPU time as tools/bench_viterbi.py: HIP events around `iters` back-to-back calls, median of 5
rounds. One JSON line per shape and K, also written to profiles/sample_align.jsonl with the source
hash bench.py's roofline uses. `met` says whether K = 1 took no longer than ssnt_fwd_bwd of the
same run (no margin); for K > 1 the ratio is information only."""
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "oracle", ROOT / "ssnt-tts-rust_amd", ROOT / "tools"):
    sys.path.insert(0, str(p))
import oracle as O  # noqa: E402
import ssnt_tts_amd as S  # noqa: E402
from bench import kernel_source_sha  # noqa: E402
from bench_viterbi import gpu_time  # noqa: E402

DEV = torch.device("cuda:0")
OUT = ROOT / "profiles" / "sample_align.jsonl"


def shape(B, T, U, Ks, iters):
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
    tf = gpu_time(lambda: S.ssnt_fwd_bwd(lt, sl, pl, need_grad=True, out=fo), iters)
    rows = []
    for K in Ks:
        gen = torch.Generator(device=DEV)
        gen.manual_seed(K)
        un = torch.rand((B, K, T), device=DEV, generator=gen)
        so = {"log_prob": torch.empty((B, K), device=DEV),
              "position": torch.empty((B, K, T), dtype=torch.int32, device=DEV),
              "duration": torch.empty((B, K, U), dtype=torch.int32, device=DEV),
              "status": torch.zeros(1, dtype=torch.int32, device=DEV)}
        S.ssnt_sample_align(lt, sl, pl, K, uniform=un, out=so, check=True)
        ts = gpu_time(lambda: S.ssnt_sample_align(lt, sl, pl, K, uniform=un, out=so, check=False), iters)
        tl = gpu_time(lambda: S.ssnt_sample_align(lt, sl, pl, K, uniform=un, need_path=False, check=False,
                                                  out={"log_prob": so["log_prob"], "status": so["status"]}), iters)
        r = {"workload": f"posterior samples B={B} T={T} U={U} K={K} (log_prob + position + duration)",
             "sample_us": ts * 1e6, "sample_log_prob_only_us": tl * 1e6, "fwd_bwd_us": tf * 1e6,
             "viterbi_us": tv * 1e6, "ratio_to_fwd_bwd": ts / tf, "ratio_to_viterbi": ts / tv,
             "workspace_bytes": int(S.load().ssnt_sample_align_workspace_size(B, T, U, K)),
             "source_sha": kernel_source_sha(), "device": torch.cuda.get_device_name(0)}
        if K == 1:
            r["met"] = {"fwd_bwd": ts <= tf}
        rows.append(r)
    return rows


def main():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", type=Path, default=OUT, help="JSON-lines file to (over)write")
    out = ap.parse_args().out
    rows = shape(256, 200, 80, (1, 4, 16), 200) + shape(64, 2000, 400, (1, 4), 20)
    out.parent.mkdir(parents=True, exist_ok=True)
    with open(out, "w") as f:
        for r in rows:
            line = json.dumps(r)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
