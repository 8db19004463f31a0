#!/usr/bin/env python3
"""Time the banded forward-backward against the dense call it was cut from, in one process on one
GPU:

  ssnt_fwd_bwd_band   B=64 T=2000 U=400 with R in {32, 64, 128}; B=256 T=200 U=80 with R in {16, 32}
  ssnt_fwd_bwd        the dense lattice of the same shape, in the same run (the yardstick)
  two-wave dense      B=64 T=2000 U=64 through the A/B build's kernel override (time per step of the
                      kernel form the banded one starts from)

The band is ssnt_band_from_positions on the Viterbi path of the dense lattice, the band tensor
ssnt_band_gather of it. GPU time as tools/bench_viterbi.py: HIP events around `iters` back-to-back
calls, median of 5 rounds. One JSON line per (shape, R), also written to
profiles/fwd_bwd_band.jsonl: both times and their ratio, microseconds per step, input + output
bytes and the rate they were moved at, both workspaces, and banded loss - dense loss (the mass the
band drops). `met` is information, not a gate."""
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
OUT = ROOT / "profiles" / "fwd_bwd_band.jsonl"


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


def dense_outs(B, T, U):
    return {"loss": torch.empty(B, device=DEV), "grad": torch.empty((B, T, U, 2), device=DEV),
            "status": torch.zeros(1, dtype=torch.int32, device=DEV)}


def two_wave_u64(B, T, iters):
    """The two-wave dense kernel at U = 64 (A/B build, kernel override 1): seconds per call."""
    lt = torch.from_numpy(O.synth_log_trans(B, T, 64, seed=0)).to(DEV)
    sl = torch.full((B,), T, dtype=torch.int32, device=DEV)
    pl = torch.full((B,), 64, dtype=torch.int32, device=DEV)
    fo = dense_outs(B, T, 64)
    with S.use_ab() as ab:
        assert ab.ssnt_fwd_bwd_set_variant(1) == 0
        S.ssnt_fwd_bwd(lt, sl, pl, out=fo, check=True)
        kernel = S.last_fwd_bwd_kernel()
        t = gpu_time(lambda: S.ssnt_fwd_bwd(lt, sl, pl, out=fo), iters)
    return t, kernel


def shape(B, T, U, widths, iters, two_wave=None):
    lt = torch.from_numpy(O.synth_log_trans(B, T, U, seed=0)).to(DEV)
    sl = torch.full((B,), T, dtype=torch.int32, device=DEV)
    pl = torch.full((B,), U, dtype=torch.int32, device=DEV)
    fo = dense_outs(B, T, U)
    S.ssnt_fwd_bwd(lt, sl, pl, out=fo, check=True)
    dense_kernel = S.last_fwd_bwd_kernel()
    td = gpu_time(lambda: S.ssnt_fwd_bwd(lt, sl, pl, out=fo), iters)
    dense_loss = fo["loss"].double().cpu().numpy()
    pos = S.ssnt_viterbi_align(lt, sl, pl, check=True)["position"]
    lib = S.load()
    rows = []
    for R in widths:
        bs = S.ssnt_band_from_positions(pos, sl, pl, R)
        band = S.ssnt_band_gather(lt, bs, R, float("-inf")).contiguous()
        bo = {"loss": torch.empty(B, device=DEV), "grad": torch.empty((B, T, R, 2), device=DEV),
              "status": torch.zeros(1, dtype=torch.int32, device=DEV)}
        S.ssnt_fwd_bwd_band(band, bs, sl, pl, out=bo, check=True)
        tb = gpu_time(lambda: S.ssnt_fwd_bwd_band(band, bs, sl, pl, out=bo), iters)
        drop = bo["loss"].double().cpu().numpy() - dense_loss
        moved = 2 * B * T * R * 8 + B * T * 4 + 3 * B * 4
        r = {"workload": f"banded fwd-bwd B={B} T={T} U={U} R={R} (loss + grad), band around the best path",
             "band_us": tb * 1e6, "dense_us": td * 1e6, "band_over_dense": tb / td,
             "band_us_per_step": tb * 1e6 / T, "dense_us_per_step": td * 1e6 / T,
             "band_bytes": moved, "band_bytes_per_s": moved / tb,
             "dense_bytes": 2 * B * T * U * 8 + 3 * B * 4, "dense_bytes_per_s": (2 * B * T * U * 8) / td,
             "band_workspace_bytes": int(lib.ssnt_fwd_bwd_band_workspace_size(B, T, R)),
             "dense_workspace_bytes": int(lib.ssnt_fwd_bwd_workspace_size(B, T, U)),
             "dense_kernel": dense_kernel,
             "loss_gap_mean": float(drop.mean()), "loss_gap_max": float(drop.max()),
             "loss_gap_min": float(drop.min()), "dense_loss_mean": float(dense_loss.mean()),
             "met": {"faster_than_dense": tb < td}}
        if two_wave is not None:
            r["two_wave_u64_us_per_step"] = two_wave[0] * 1e6 / T
            r["two_wave_u64_kernel"] = two_wave[1]
            if R == 64:
                r["met"]["step_no_slower_than_two_wave_u64"] = tb <= two_wave[0]
        r["source_sha"] = kernel_source_sha()
        r["device"] = torch.cuda.get_device_name(0)
        rows.append(r)
    return rows


def main():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", type=Path, default=OUT, help="JSON-lines file to (over)write")
    out = ap.parse_args().out
    tw = two_wave_u64(64, 2000, 20)
    rows = shape(64, 2000, 400, (32, 64, 128), 20, two_wave=tw) + shape(256, 200, 80, (16, 32), 200)
    out.parent.mkdir(parents=True, exist_ok=True)
    with open(out, "w") as f:
        for r in rows:
            line = json.dumps(r)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
