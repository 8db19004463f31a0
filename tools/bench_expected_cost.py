#!/usr/bin/env python3
"""Measure the expected path cost on the emit/shift lattice (ssnt_expected_cost), in one process on
one GPU.

Timing (default; profiles/expected_cost.jsonl), at B=256 T=200 U=80 and B=64 T=2000 U=400:

  ssnt_expected_cost(need_grad=False)  the value-only call: one forward chain
  ssnt_expected_cost                   the full call: both sweeps, then the gradient launch; the
                                       two launches also alone (the A/B build's launch mask, over
                                       the workspace a full call left)
  ssnt_fwd_bwd(need_grad)              the same shapes
  ssnt_sample_align, one sample        the same forward chain structure (log_prob + path)

GPU time as tools/bench_viterbi.py: HIP events around `iters` back-to-back calls, median of 5
rounds. `expectation` records whether the value-only call took no longer than 1.25x the one-sample
sampler of the same run (information, not a gate).

--accuracy (profiles/expected_cost_accuracy.jsonl): every case of tests/expected_cost_cases.py plus
the two shapes above (N(0,1) costs, then the entropy cost) against the float64 reference
tests/expected_cost_ref.py, normalised as tests/expected_cost_cases.py `errors` does; at the two
large shapes the kernel runs the whole batch and the first few utterances are compared. One line
per case, then one line "worst" with the largest value per output and the case it came from: the
tests' tolerances are 4x those, rounded up to one significant digit. `ceiling` is S * 2^-24 of the
case: a larger normalised error is a bug, not a tolerance."""
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
OUT = ROOT / "profiles" / "expected_cost.jsonl"
OUT_ACC = ROOT / "profiles" / "expected_cost_accuracy.jsonl"
SHAPES = ((256, 200, 80, 200, 8), (64, 2000, 400, 20, 4))  # B, T, U, timing iters, utterances compared


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_case(c, need_grad=True):
    r = S.ssnt_expected_cost(_t(c["lt"]), _t(c["cost"]), _t(c["S"]), _t(c["P"]), _t(c["lo"]),
                             terminal_emit=c["terminal"], need_grad=need_grad, check=False)
    return {k: v.cpu().numpy() for k, v in r.items()}


def accuracy(out):
    import expected_cost_cases as EC
    ab = S.load_ab()
    cases = EC.all_cases(lambda U, obs: ab.ssnt_expected_cost_chunk_rows(U, int(obs)))
    rows = []

    def one(name, c, keep=None):
        got = run_case(c)
        if keep is not None:  # the whole batch ran; the first `keep` utterances are compared
            c = {k: (v[:keep] if isinstance(v, np.ndarray) else v) for k, v in c.items()}
            got = {k: (v[:keep] if k != "status" else v) for k, v in got.items()}
        ref = EC.reference(c)
        e = EC.errors(got, ref)
        smax = int(max(c["S"].max(), 1))
        rows.append({"case": name, "shape": list(c["lt"].shape[:3]), "errors": e,
                     "ceiling": smax * 2.0 ** -24, "above_ceiling": [k for k, v in e.items() if not v <= smax * 2.0 ** -24]})

    for name, c in cases.items():
        one(name, c)
    for B, T, U, _, keep in SHAPES:
        for kind in ("normal", "entropy"):
            c = EC.make(B, T, U, T, obs=False, S=[T] * B, P=[U] * B)
            if kind == "entropy":
                c["cost"] = c["lt"].copy()
            one(f"large-B{B}-T{T}-U{U}-{kind}", c, keep)
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
    for B, T, U, iters, _ in SHAPES:
        lt = torch.from_numpy(O.synth_log_trans(B, T, U, seed=0)).to(DEV)
        cost = torch.randn((B, T, U, 2), device=DEV)
        sl = torch.full((B,), T, dtype=torch.int32, device=DEV)
        pl = torch.full((B,), U, dtype=torch.int32, device=DEV)
        f32 = {"device": DEV, "dtype": torch.float32}
        st = torch.zeros(1, dtype=torch.int32, device=DEV)
        vo = {"risk": torch.empty(B, **f32), "loss": torch.empty(B, **f32), "status": st}
        eo = dict(vo, grad_trans=torch.empty((B, T, U, 2), **f32), grad_cost=torch.empty((B, T, U, 2), **f32))
        fo = {"loss": torch.empty(B, **f32), "grad": torch.empty((B, T, U, 2), **f32), "status": st}
        so = {"log_prob": torch.empty((B, 1), **f32), "position": torch.empty((B, 1, T), dtype=torch.int32, device=DEV),
              "duration": torch.empty((B, 1, U), dtype=torch.int32, device=DEV), "status": st}
        un = torch.rand((B, 1, T), device=DEV)
        S.ssnt_expected_cost(lt, cost, sl, pl, out=eo, check=True)
        S.ssnt_fwd_bwd(lt, sl, pl, out=fo, check=True)
        S.ssnt_sample_align(lt, sl, pl, 1, uniform=un, out=so, check=True)
        tv = gpu_time(lambda: S.ssnt_expected_cost(lt, cost, sl, pl, need_grad=False, out=vo), iters)
        te = gpu_time(lambda: S.ssnt_expected_cost(lt, cost, sl, pl, out=eo), iters)
        tf = gpu_time(lambda: S.ssnt_fwd_bwd(lt, sl, pl, need_grad=True, out=fo), iters)
        ts = gpu_time(lambda: S.ssnt_sample_align(lt, sl, pl, 1, uniform=un, out=so, check=False), iters)
        # one launch at a time, over the workspace of one buffer (torch's allocator hands the same
        # block back to every call of this loop)
        part = {}
        with S.use_ab():
            S.ssnt_expected_cost(lt, cost, sl, pl, out=eo, check=True)
            for name, mask in (("sweep", 1), ("grad", 2)):
                ab.ssnt_expected_cost_launches(mask)
                part[name] = gpu_time(lambda: S.ssnt_expected_cost(lt, cost, sl, pl, out=eo), iters)
            ab.ssnt_expected_cost_launches(3)
        cells = B * T * U
        rows.append({"workload": f"expected path cost B={B} T={T} U={U} (no log_obs)",
                     "value_only_us": tv * 1e6, "full_us": te * 1e6, "sweep_us": part["sweep"] * 1e6,
                     "grad_launch_us": part["grad"] * 1e6, "fwd_bwd_us": tf * 1e6, "sample1_us": ts * 1e6,
                     "value_only_to_sample1": tv / ts, "full_to_fwd_bwd": te / tf,
                     "grad_launch_GBps": cells * (32 + 24) / part["grad"] / 1e9,
                     "workspace_bytes": int(S.load().ssnt_expected_cost_workspace_size(B, T, U)),
                     "expectation": {"value_only_about_sample1": tv <= 1.25 * ts},
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
