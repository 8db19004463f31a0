#!/usr/bin/env python3
"""Time the banded best path against its three yardsticks, in one process on one GPU:

  ssnt_viterbi_align_band  B=64 T=2000 U=400 with R in {32, 64, 128}; B=256 T=200 U=80 with R in {16, 32}
  (a) ssnt_viterbi_align   the dense lattice of the shape
  (b) ssnt_fwd_bwd_band    need_grad=False, on the same band
  (c) ssnt_viterbi_align   a dense lattice with U = R and the same T: the scaffold's own step, no band

The band is ssnt_band_from_positions on the dense best path of oracle.synth_log_trans, the band
tensor ssnt_band_gather of it. GPU time as tools/bench_fwd_bwd_band.py: HIP events around `iters`
back-to-back calls, median of 5 rounds; every yardstick is measured in this run. One JSON line
per (shape, R), also written to profiles/viterbi_align_band.jsonl: the four times with the spread
(max - min) of their rounds, the ratios, microseconds per step, the workspace, and whether the
banded path is the dense one. The banded call and (c) are also timed with need_path=False: the
sweeps alone, since (c) walks R positions where the band walks the utterance's P. `met` is
information, not a gate."""
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
OUT = ROOT / "profiles" / "viterbi_align_band.jsonl"


def gpu_time(fn, iters, rounds=5):
    """(median, max - min) of `rounds` timings of `iters` back-to-back calls, seconds per call."""
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
    return float(np.median(ts)), float(max(ts) - min(ts))


def path_outs(B, T, U):
    return {"log_prob": torch.empty(B, device=DEV), "position": torch.empty((B, T), dtype=torch.int32, device=DEV),
            "duration": torch.empty((B, U), dtype=torch.int32, device=DEV),
            "status": torch.zeros(1, dtype=torch.int32, device=DEV)}


def shape(B, T, U, widths, iters):
    lt = torch.from_numpy(O.synth_log_trans(B, T, U, seed=0)).to(DEV)
    sl = torch.full((B,), T, dtype=torch.int32, device=DEV)
    pl = torch.full((B,), U, dtype=torch.int32, device=DEV)
    do = path_outs(B, T, U)
    S.ssnt_viterbi_align(lt, sl, pl, out=do, check=True)
    ta, sa = gpu_time(lambda: S.ssnt_viterbi_align(lt, sl, pl, out=do), iters)
    pos = do["position"].clone()
    lib = S.load()
    rows = []
    for R in widths:
        bs = S.ssnt_band_from_positions(pos, sl, pl, R)
        band = S.ssnt_band_gather(lt, bs, R, float("-inf")).contiguous()
        bo = path_outs(B, T, U)
        S.ssnt_viterbi_align_band(band, bs, sl, pl, max_pos=U, out=bo, check=True)
        same = bool(torch.equal(bo["position"], pos)) and bool(torch.equal(bo["log_prob"], do["log_prob"]))
        contact = S.ssnt_band_edge_contact(bo["position"], bs, sl, pl, R)
        tv, sv = gpu_time(lambda: S.ssnt_viterbi_align_band(band, bs, sl, pl, max_pos=U, out=bo), iters)
        lo_ = {"log_prob": bo["log_prob"], "status": bo["status"]}
        tl, sl_ = gpu_time(lambda: S.ssnt_viterbi_align_band(band, bs, sl, pl, need_path=False, out=lo_), iters)
        fo = {"loss": torch.empty(B, device=DEV), "status": torch.zeros(1, dtype=torch.int32, device=DEV)}
        S.ssnt_fwd_bwd_band(band, bs, sl, pl, need_grad=False, out=fo, check=True)
        tb, sb = gpu_time(lambda: S.ssnt_fwd_bwd_band(band, bs, sl, pl, need_grad=False, out=fo), iters)
        # (c): a dense lattice of R positions, every one of them live
        ltc = torch.from_numpy(O.synth_log_trans(B, T, R, seed=1)).to(DEV)
        plc = torch.full((B,), min(R, T), dtype=torch.int32, device=DEV)
        co = path_outs(B, T, R)
        S.ssnt_viterbi_align(ltc, sl, plc, out=co, check=True)
        tc, sc = gpu_time(lambda: S.ssnt_viterbi_align(ltc, sl, plc, out=co), iters)
        # the sweeps alone (no words, no walk): (c) walks R positions, the band the utterance's P
        cl = {"log_prob": co["log_prob"], "status": co["status"]}
        tcl, scl = gpu_time(lambda: S.ssnt_viterbi_align(ltc, sl, plc, need_path=False, out=cl), iters)
        r = {"workload": f"banded best path B={B} T={T} U={U} R={R} (log_prob + position + duration), "
                         "band around the dense best path",
             "band_us": tv * 1e6, "band_spread_us": sv * 1e6, "band_log_prob_only_us": tl * 1e6,
             "dense_us": ta * 1e6, "dense_spread_us": sa * 1e6,
             "fwd_bwd_band_loss_us": tb * 1e6, "fwd_bwd_band_spread_us": sb * 1e6,
             "dense_u_eq_r_us": tc * 1e6, "dense_u_eq_r_spread_us": sc * 1e6,
             "band_log_prob_only_spread_us": sl_ * 1e6,
             "dense_u_eq_r_log_prob_only_us": tcl * 1e6, "dense_u_eq_r_log_prob_only_spread_us": scl * 1e6,
             "band_over_dense": tv / ta, "band_over_fwd_bwd_band": tv / tb, "band_over_dense_u_eq_r": tv / tc,
             "sweep_over_dense_u_eq_r_sweep": tl / tcl,
             "band_us_per_step": tv * 1e6 / T, "dense_u_eq_r_us_per_step": tc * 1e6 / T,
             "band_sweep_us_per_step": tl * 1e6 / T, "dense_u_eq_r_sweep_us_per_step": tcl * 1e6 / T,
             "band_bytes": B * T * R * 8 + 2 * B * T * 4 + B * U * 4, "dense_bytes": B * T * U * 8,
             "band_workspace_bytes": int(lib.ssnt_viterbi_align_band_workspace_size(B, T, R)),
             "dense_workspace_bytes": int(lib.ssnt_viterbi_align_workspace_size(B, T, U)),
             "same_path_and_log_prob_as_dense": same,
             "edge_contact_mean": float(contact.float().mean()), "edge_contact_max": int(contact.max()),
             "met": {"faster_than_dense": tv < ta, "faster_than_fwd_bwd_band_loss": tv < tb,
                     "step_within_spread_of_dense_u_eq_r": tv - tc <= max(sv, sc),
                     "sweep_within_spread_of_dense_u_eq_r": tl - tcl <= max(sl_, scl)},
             "source_sha": kernel_source_sha(), "device": torch.cuda.get_device_name(0)}
        rows.append(r)
    return rows


def main():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", type=Path, default=OUT, help="JSON-lines file to (over)write")
    out = ap.parse_args().out
    rows = shape(64, 2000, 400, (32, 64, 128), 20) + shape(256, 200, 80, (16, 32), 200)
    out.parent.mkdir(parents=True, exist_ok=True)
    with open(out, "w") as f:
        for r in rows:
            line = json.dumps(r)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
