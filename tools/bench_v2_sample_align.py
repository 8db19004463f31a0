#!/usr/bin/env python3
"""Time posterior sampling on the v2 lattice against its yardsticks, in one process on one GPU, at
the configs[4] shape (B=64 I=400 O=2000 D=16), band mode and test mode, K = 1, 4, 16, 64 samples:

  v2_sample_align                   log_prob + duration_class + duration + total (two launches)
  v2_fwd_bwd(need_grad=False)       the sum over the same lattice (both sweeps)
  v2_viterbi_align                  the best path over the same lattice

Each launch of the sampler is also timed on its own, and the walk in each of its forms (one gather
per step; two / four steps per memory round trip), through the A/B build's
ssnt_v2_sample_align_form: a walk alone runs over the rows the preceding full call left in the
same workspace. GPU time as tools/bench_v2_viterbi.py: HIP events around `iters` back-to-back
calls, median of 5 rounds. One JSON line per (mode, K), also written to
profiles/v2_sample_align.jsonl with the source hash bench.py's roofline uses. The yardstick: at
K = 16 the walk takes no longer than the forward launch, i.e. the call <= 2 x
v2_fwd_bwd(need_grad=False) of the same run (`met`)."""
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
OUT = ROOT / "profiles" / "v2_sample_align.jsonl"


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


def mode(test_mode, iters, B=64, I=400, Ot=2000, D=16, samples=(1, 4, 16, 64)):
    d = O.synth_durations(B, I, Ot, D, seed=0)
    lg = torch.from_numpy(O.synth_v2_step_logits(d, D, seed=1)).to(DEV)
    table = torch.arange(D, dtype=torch.int32, device=DEV)
    il = torch.full((B,), I, dtype=torch.int32, device=DEV)
    ol = torch.full((B,), Ot, dtype=torch.int32, device=DEV)
    kw = dict(allow_skip=False, test_mode=test_mode, max_total=Ot)
    vo = {"log_prob": torch.empty(B, device=DEV),
          "duration_class": torch.empty((B, I), dtype=torch.int32, device=DEV),
          "duration": torch.empty((B, I), dtype=torch.int32, device=DEV),
          "total": torch.empty(B, dtype=torch.int32, device=DEV),
          "status": torch.zeros(1, dtype=torch.int32, device=DEV)}
    S.v2_fwd_bwd(lg, table, il, ol, 0, need_grad=False, check=True, **kw)
    tf = gpu_time(lambda: S.v2_fwd_bwd(lg, table, il, ol, 0, need_grad=False, **kw), iters)
    tv = gpu_time(lambda: S.v2_viterbi_align(lg, table, il, ol, 0, out=vo, **kw), iters)
    rows = []
    for K in samples:
        un = torch.rand((B, K, I + 1), device=DEV, generator=torch.Generator(device=DEV).manual_seed(K))
        so = {"log_prob": torch.empty((B, K), device=DEV),
              "duration_class": torch.empty((B, K, I), dtype=torch.int32, device=DEV),
              "duration": torch.empty((B, K, I), dtype=torch.int32, device=DEV),
              "total": torch.empty((B, K), dtype=torch.int32, device=DEV),
              "status": torch.zeros(1, dtype=torch.int32, device=DEV)}

        def call():
            return S.v2_sample_align(lg, table, il, ol, 0, K, uniform=un, out=so, **kw)

        S.v2_sample_align(lg, table, il, ol, 0, K, uniform=un, out=so, check=True, **kw)
        assert bool(torch.all(torch.isfinite(so["log_prob"])))
        want = {k: so[k].clone() for k in ("log_prob", "duration_class", "total")}
        tc = gpu_time(call, iters)
        forms = {}
        with S.use_ab() as ab:
            call()  # the rows the walk-only runs read: this workspace block, reused by the allocator
            assert ab.ssnt_v2_sample_align_form(0, 1) == 0
            t_fwd = gpu_time(call, iters)
            for name, cone in (("auto", 0), ("gather", 1), ("cone2", 2), ("cone4", 4)):
                assert ab.ssnt_v2_sample_align_form(cone, 3) == 0
                call()
                assert ab.ssnt_v2_sample_align_form(cone, 2) == 0
                forms[name] = gpu_time(call, iters)
                torch.cuda.synchronize()
                for k, v in want.items():  # every form draws the same bits
                    assert torch.equal(so[k], v), (name, k)
        rows.append({"workload": f"v2 posterior samples B={B} I={I} O={Ot} D={D} K={K} "
                                 f"{'test' if test_mode else 'band'} mode "
                                 "(log_prob + duration_class + duration + total)",
                     "test_mode": bool(test_mode), "num_samples": K,
                     "sample_us": tc * 1e6, "forward_launch_us": t_fwd * 1e6, "walk_launch_us": forms["auto"] * 1e6,
                     "walk_gather_us": forms["gather"] * 1e6, "walk_cone2_us": forms["cone2"] * 1e6,
                     "walk_cone4_us": forms["cone4"] * 1e6,
                     "fwd_bwd_no_grad_us": tf * 1e6, "viterbi_us": tv * 1e6,
                     "ratio_to_fwd_bwd": tc / tf, "walk_to_forward": forms["auto"] / t_fwd,
                     "workspace_bytes": int(S.load().ssnt_v2_sample_align_workspace_size(B, I, Ot, test_mode, K)),
                     "met": {"call_le_2x_fwd_bwd": tc <= 2 * tf, "walk_le_forward": forms["auto"] <= t_fwd},
                     "source_sha": kernel_source_sha(), "device": torch.cuda.get_device_name(0)})
    return rows


def main():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", type=Path, default=OUT, help="JSON-lines file to (over)write")
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    rows = mode(False, a.iters) + mode(True, a.iters)
    a.out.parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            line = json.dumps(r)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
