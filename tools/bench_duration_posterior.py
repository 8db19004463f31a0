#!/usr/bin/env python3
"""Measure the posterior duration distribution on the emit/shift lattice
(ssnt_duration_posterior), in one process on one GPU.

Timing (default; profiles/duration_posterior.jsonl), at B=256 T=200 U=80 D=32 and B=64 T=2000 U=400
D=64:

  ssnt_duration_posterior   the whole call: both sweeps (alpha and beta rows, no mean), then the
                            duration launch; the two launches also alone (the A/B build's launch
                            mask, over the workspace a full call left)
  ssnt_expected_cost        the full call with gradients: the yardstick
  ssnt_fwd_bwd(need_grad)   the same shapes

GPU time as tools/bench_viterbi.py: HIP events around `iters` back-to-back calls, median of 5
rounds. `expectation` records whether the whole call took no longer than the full
ssnt_expected_cost call of the same run (information, not a gate). The duration launch's achieved
bytes/s count 24 B per cell read (alpha and beta rows 16, log_trans 8; no log_obs here) plus dur_post
written; its arithmetic rate counts 3 flops (two multiplies, one add) per cell of the band and bin
lane the form carries.

--accuracy (profiles/duration_posterior_accuracy.jsonl): every case of
tests/duration_posterior_cases.py plus the two shapes above against the float64 reference
tests/duration_posterior_ref.py, as tests/duration_posterior_cases.py `errors` has them; at the two
large shapes the kernel runs the whole batch and the first 8 / 4 utterances are compared. One line
per case, then one line "worst" with the largest value per output and the case it came from: the
tests' tolerances are 4x those, rounded up to one significant digit."""
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "oracle", ROOT / "ssnt-tts-rust_amd", ROOT / "tools", ROOT / "tests"):
    sys.path.insert(0, str(p))
import ssnt_tts_amd as S  # noqa: E402
from bench import kernel_source_sha  # noqa: E402
from bench_viterbi import gpu_time  # noqa: E402

DEV = torch.device("cuda:0")
OUT = ROOT / "profiles" / "duration_posterior.jsonl"
OUT_ACC = ROOT / "profiles" / "duration_posterior_accuracy.jsonl"
SHAPES = ((256, 200, 80, 32, 200, 8), (64, 2000, 400, 64, 20, 4))  # B, T, U, D, timing iters, utterances compared
VALU_PEAK_FLOPS = 256 * 4 * 16 * 2 * 2.4e9  # CUs x SIMDs x lanes x (fma = 2) x clock: plain f32 VALU


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_case(c):
    r = S.ssnt_duration_posterior(_t(c["lt"]), _t(c["S"]), _t(c["P"]), c["D"], _t(c["lo"]),
                                  terminal_emit=c["terminal"], check=False)
    return {k: v.cpu().numpy() for k, v in r.items()}


def block():
    blk = S.load_ab().ssnt_duration_posterior_block(64, 32, 0)
    return blk & 0xFFFF, blk >> 16


def accuracy(out):
    import duration_posterior_cases as DC
    ab = S.load_ab()
    cases = DC.all_cases(*block(), lambda U, obs: ab.ssnt_duration_posterior_sweep_rows(U, int(obs)))
    rows = []

    def one(name, c, keep=None):
        got = run_case(c)
        if keep is not None:  # the whole batch ran; the first `keep` utterances are compared
            c = {k: (v[:keep] if isinstance(v, np.ndarray) else v) for k, v in c.items()}
            got = {k: (v[:keep] if k != "status" else v) for k, v in got.items()}
        ref = DC.reference(c)
        e = DC.errors(got, ref)
        exact = not np.ascontiguousarray(got["dur_post"][DC.impossible(c)]).view(np.uint32).any()
        rows.append({"case": name, "shape": list(c["lt"].shape[:3]) + [c["D"]], "errors": e,
                     "impossible_bins_zero": bool(exact)})

    for name, c in cases.items():
        one(name, c)
    for B, T, U, D, _, keep in SHAPES:
        one(f"large-B{B}-T{T}-U{U}-D{D}", DC.make(B, T, U, D, T, obs=False, S=[T] * B, P=[U] * B), keep)
    worst = {}
    for r in rows:
        for k, v in r["errors"].items():
            if k not in worst or not v <= worst[k]["value"]:
                worst[k] = {"value": v, "case": r["case"]}
    rows.append({"case": "worst", "errors": worst, "source_sha": kernel_source_sha(),
                 "device": torch.cuda.get_device_name(0)})
    write(out, rows)


def timing(out):
    import oracle as O
    ab = S.load_ab()
    rows = []
    for B, T, U, D, iters, _ in SHAPES:
        lt = torch.from_numpy(O.synth_log_trans(B, T, U, seed=0)).to(DEV)
        cost = torch.randn((B, T, U, 2), device=DEV)
        sl = torch.full((B,), T, dtype=torch.int32, device=DEV)
        pl = torch.full((B,), U, dtype=torch.int32, device=DEV)
        f32 = {"device": DEV, "dtype": torch.float32}
        st = torch.zeros(1, dtype=torch.int32, device=DEV)
        do = {"dur_post": torch.empty((B, U, D), **f32), "loss": torch.empty(B, **f32), "status": st}
        eo = {"risk": torch.empty(B, **f32), "loss": torch.empty(B, **f32), "status": st,
              "grad_trans": torch.empty((B, T, U, 2), **f32), "grad_cost": torch.empty((B, T, U, 2), **f32)}
        fo = {"loss": torch.empty(B, **f32), "grad": torch.empty((B, T, U, 2), **f32), "status": st}
        S.ssnt_duration_posterior(lt, sl, pl, D, out=do, check=True)
        S.ssnt_expected_cost(lt, cost, sl, pl, out=eo, check=True)
        S.ssnt_fwd_bwd(lt, sl, pl, out=fo, check=True)
        td = gpu_time(lambda: S.ssnt_duration_posterior(lt, sl, pl, D, out=do, check=False), iters)
        te = gpu_time(lambda: S.ssnt_expected_cost(lt, cost, sl, pl, out=eo), iters)
        tf = gpu_time(lambda: S.ssnt_fwd_bwd(lt, sl, pl, need_grad=True, out=fo), iters)
        # one launch at a time, over the workspace of one buffer (torch's allocator hands the same
        # block back to every call of this loop)
        part = {}
        with S.use_ab():
            S.ssnt_duration_posterior(lt, sl, pl, D, out=do, check=True)
            for name, mask in (("sweeps", 1), ("duration", 2)):
                ab.ssnt_duration_posterior_launches(mask)
                part[name] = gpu_time(lambda: S.ssnt_duration_posterior(lt, sl, pl, D, out=do, check=False), iters)
            ab.ssnt_duration_posterior_launches(3)
        cells = B * T * U
        band = B * (T - U + 1) * U                   # cells inside a position's band
        lanes = 16 if D - 1 <= 16 else 32 if D - 1 <= 32 else 64 if D - 1 <= 64 else 128 if D - 1 <= 128 else 256
        rows.append({"workload": f"duration posterior B={B} T={T} U={U} D={D} (no log_obs)",
                     "full_us": td * 1e6, "sweeps_us": part["sweeps"] * 1e6, "duration_launch_us": part["duration"] * 1e6,
                     "expected_cost_full_us": te * 1e6, "fwd_bwd_us": tf * 1e6, "full_to_expected_cost": td / te,
                     "duration_launch_GBps": (cells * 24 + B * U * D * 4) / part["duration"] / 1e9,
                     "duration_launch_GFLOPs": band * lanes * 3 / part["duration"] / 1e9,
                     "duration_launch_valu_share": band * lanes * 3 / part["duration"] / VALU_PEAK_FLOPS,
                     "workspace_bytes": int(S.load().ssnt_duration_posterior_workspace_size(B, T, U, D)),
                     "expectation": {"no_slower_than_expected_cost": td <= te},
                     "source_sha": kernel_source_sha(), "device": torch.cuda.get_device_name(0)})
    write(out, rows)


def write(out, rows):
    out.parent.mkdir(parents=True, exist_ok=True)
    with open(out, "w") as f:
        for r in rows:
            line = json.dumps(r)
            print(line)
            f.write(line + "\n")


def main():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--accuracy", action="store_true", help="measure errors against the float64 reference")
    ap.add_argument("--out", type=Path, default=None, help="JSON-lines file to (over)write")
    a = ap.parse_args()
    if a.accuracy:
        accuracy(a.out or OUT_ACC)
    else:
        timing(a.out or OUT)


if __name__ == "__main__":
    main()
