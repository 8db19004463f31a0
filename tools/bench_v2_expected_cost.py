#!/usr/bin/env python3
"""Measure the expected path cost on the v2 duration-class lattice (v2_expected_cost), in one
process on one GPU.

Timing (default; profiles/v2_expected_cost.jsonl), at B=64 I=400 O=2000 D=16 in band mode and in
test mode, all within one run:

  v2_expected_cost(need_grad=False)  the value-only call: the forward sweep alone, nothing stored
  v2_expected_cost                   the full call: both sweeps, then the gradient launch; the two
                                     launches also alone (the A/B build's launch mask, over the
                                     workspace a full call left)
  v2_fwd_bwd(need_grad)              the same shapes: F4, whose sweep and gradient launch these are

GPU time as tools/bench_viterbi.py: HIP events around `iters` back-to-back calls, median of 5
rounds. `expectation` records whether the mean costs the sweep much less than its share of the
instructions (information, not a gate).

--parent-lib PATH adds the regression check of v2_fwd_bwd: the same two shapes timed through the
library at PATH (a build of the parent commit) and through the product library, each in its own
child process, alternating, medians over the rounds.

--accuracy (profiles/v2_expected_cost_accuracy.jsonl): every case of
tests/v2_expected_cost_cases.py plus the shape above in band and test mode (N(0,1) costs, then the
entropy cost) against the float64 reference tests/v2_expected_cost_ref.py, normalised as
tests/v2_expected_cost_cases.py `errors` does; at the large shape the kernel runs the whole batch
and the first 8 of its 64 utterances are compared. One line per case, then one line "worst" with the
largest value per output and the case it came from: the tests' tolerances are 4x those, rounded up
to one significant digit. A worst value above 1e-5 is a defect in the arithmetic."""
import ctypes
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "oracle", ROOT / "ssnt-tts-rust_amd", ROOT / "tools", ROOT / "tests"):
    sys.path.insert(0, str(p))

DEV = torch.device("cuda:0")
OUT = ROOT / "profiles" / "v2_expected_cost.jsonl"
OUT_ACC = ROOT / "profiles" / "v2_expected_cost_accuracy.jsonl"
B, I, O, D = 64, 400, 2000, 16
ITERS, KEEP = 20, 8  # KEEP: utterances of the large shape compared with the float64 reference
NORTH_STAR = 1e-5


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def large_case(test_mode, kind="random"):
    import v2_expected_cost_cases as EC
    rng = np.random.default_rng(400)
    logits = np.log(rng.dirichlet(np.ones(D), size=(B, I))).astype(np.float32)
    c = EC.make(logits, [I] * B, [O] * B, np.arange(D), mt=O, allow_skip=True, test_mode=test_mode, seed=400)
    if kind == "entropy":
        c["cost"] = c["logits"].copy()
    return c


def run_case(S, c, need_grad=True):
    r = S.v2_expected_cost(_t(c["logits"]), _t(c["cost"]), _t(c["table"], torch.int32), _t(c["I"], torch.int32),
                           _t(c["O"], torch.int32), c["zid"], allow_skip=c["allow_skip"], test_mode=c["test_mode"],
                           max_total=c["mt"], need_grad=need_grad, check=False)
    return {k: v.cpu().numpy() for k, v in r.items()}


def accuracy(out):
    import ssnt_tts_amd as S
    import v2_expected_cost_cases as EC
    from bench import kernel_source_sha
    ab = S.load_ab()
    cases = EC.all_cases(lambda d: ab.ssnt_v2_expected_cost_chunk_steps(d))
    rows = []

    def one(name, c, keep=None):
        got = run_case(S, c)
        if keep is not None:  # the whole batch ran; the first `keep` utterances are compared
            c = {k: (v[:keep] if k in ("logits", "cost", "I", "O") else v) for k, v in c.items()}
            got = {k: (v[:keep] if k != "status" else v) for k, v in got.items()}
        e = EC.errors(got, EC.reference(c))
        rows.append({"case": name, "shape": list(c["logits"].shape), "utterances_compared": len(c["I"]), "errors": e,
                     "above_1e-5": [k for k, v in e.items() if not v <= NORTH_STAR]})

    for name, c in cases.items():
        one(name, c)
    for tm in (False, True):
        for kind in ("random", "entropy"):
            one(f"large-B{B}-I{I}-O{O}-D{D}-{'test' if tm else 'band'}-{kind}", large_case(tm, kind), KEEP)
    worst = {}
    for r in rows:
        for k, v in r["errors"].items():
            if k not in worst or not v <= worst[k]["value"]:
                worst[k] = {"value": v, "case": r["case"]}
    rows.append({"case": "worst", "errors": worst, "source_sha": kernel_source_sha(),
                 "device": torch.cuda.get_device_name(0)})
    write(out, rows)


def timing(out, parent_lib):
    import ssnt_tts_amd as S
    from bench import kernel_source_sha
    from bench_viterbi import gpu_time
    ab = S.load_ab()
    rows = []
    for tm in (False, True):
        c = large_case(tm)
        lg, cs = _t(c["logits"]), _t(c["cost"])
        tb, il, ol = _t(c["table"], torch.int32), _t(c["I"], torch.int32), _t(c["O"], torch.int32)
        kw = dict(allow_skip=True, test_mode=tm, max_total=O)
        f32 = {"device": DEV, "dtype": torch.float32}
        st = torch.zeros(1, dtype=torch.int32, device=DEV)
        vo = {"risk": torch.empty(B, **f32), "loss": torch.empty(B, **f32), "status": st}
        eo = dict(vo, grad_logits=torch.empty((B, I, D), **f32), grad_cost=torch.empty((B, I, D), **f32))
        fo = {"loss": torch.empty(B, **f32), "grad": torch.empty((B, I, D), **f32), "status": st}
        fv = {"loss": torch.empty(B, **f32), "status": st}
        S.v2_expected_cost(lg, cs, tb, il, ol, 0, out=eo, check=True, **kw)
        S.v2_fwd_bwd(lg, tb, il, ol, 0, out=fo, check=True, **kw)
        tv = gpu_time(lambda: S.v2_expected_cost(lg, cs, tb, il, ol, 0, need_grad=False, out=vo, **kw), ITERS)
        te = gpu_time(lambda: S.v2_expected_cost(lg, cs, tb, il, ol, 0, out=eo, **kw), ITERS)
        tfv = gpu_time(lambda: S.v2_fwd_bwd(lg, tb, il, ol, 0, need_grad=False, out=fv, **kw), ITERS)
        tf = gpu_time(lambda: S.v2_fwd_bwd(lg, tb, il, ol, 0, need_grad=True, out=fo, **kw), ITERS)
        # one launch at a time, over the workspace of one buffer (torch's allocator hands the same
        # block back to every call of this loop)
        part = {}
        with S.use_ab():
            S.v2_expected_cost(lg, cs, tb, il, ol, 0, out=eo, check=True, **kw)
            for name, mask in (("sweep", 1), ("grad", 2)):
                ab.ssnt_v2_expected_cost_launches(mask)
                part[name] = gpu_time(lambda: S.v2_expected_cost(lg, cs, tb, il, ol, 0, out=eo, **kw), ITERS)
            ab.ssnt_v2_expected_cost_launches(3)
        f4_grad = tf - tfv  # (F4's gradient launch: the full call less its sweeps)
        lib = S.load()
        rows.append({"workload": f"v2 expected path cost B={B} I={I} O={O} D={D} {'test' if tm else 'band'} mode",
                     "value_only_us": tv * 1e6, "full_us": te * 1e6, "sweep_us": part["sweep"] * 1e6,
                     "grad_launch_us": part["grad"] * 1e6, "f4_value_only_us": tfv * 1e6, "f4_full_us": tf * 1e6,
                     "f4_grad_launch_us_by_difference": f4_grad * 1e6,
                     "value_only_to_f4_value_only": tv / tfv, "full_to_f4_full": te / tf,
                     "sweeps_to_f4_sweeps": part["sweep"] / tfv, "grad_launch_to_f4": part["grad"] / f4_grad,
                     "workspace_bytes": int(lib.ssnt_v2_expected_cost_workspace_size(B, I, O, tm, True)),
                     "f4_workspace_bytes": int(lib.ssnt_v2_fwd_bwd_workspace_size(B, I, O, tm)),
                     "expectation": {"sweep_costs_much_less_than_its_instruction_share": part["sweep"] / tfv <= 1.25},
                     "source_sha": kernel_source_sha(), "device": torch.cuda.get_device_name(0)})
    if parent_lib:
        rows.append(regression(parent_lib))
    write(out, rows)


def f4_child(lib_path):
    """v2_fwd_bwd of the library at lib_path through ctypes alone (a parent build lacks the newer
    symbols the package binds): one JSON line of median microseconds, band and test mode."""
    from bench_viterbi import gpu_time
    lib = ctypes.CDLL(lib_path)
    lib.ssnt_v2_fwd_bwd_workspace_size.restype = ctypes.c_size_t
    lib.ssnt_v2_fwd_bwd_workspace_size.argtypes = [ctypes.c_int] * 3 + [ctypes.c_bool]
    P = ctypes.c_void_p
    lib.ssnt_v2_fwd_bwd_device.restype = ctypes.c_int
    lib.ssnt_v2_fwd_bwd_device.argtypes = [P, P, P, P] + [ctypes.c_int] * 5 + [ctypes.c_bool] * 2 + [ctypes.c_int] + \
        [P] * 5 + [ctypes.c_size_t, P, P]
    res = {}
    for tm in (False, True):
        c = large_case(tm)
        lg = _t(c["logits"])
        tb, il, ol = _t(c["table"], torch.int32), _t(c["I"], torch.int32), _t(c["O"], torch.int32)
        loss, grad = torch.empty(B, device=DEV), torch.empty((B, I, D), device=DEV)
        st = torch.zeros(1, dtype=torch.int32, device=DEV)
        wsb = lib.ssnt_v2_fwd_bwd_workspace_size(B, I, O, tm)
        ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
        stream = torch.cuda.current_stream().cuda_stream

        def call():
            rc = lib.ssnt_v2_fwd_bwd_device(lg.data_ptr(), tb.data_ptr(), il.data_ptr(), ol.data_ptr(), B, I, D, O, 0,
                                            True, tm, 0, loss.data_ptr(), grad.data_ptr(), None, None, ws.data_ptr(),
                                            wsb, st.data_ptr(), stream)
            assert rc == 0, rc

        res["test" if tm else "band"] = {"us": gpu_time(call, ITERS) * 1e6,
                                         "checksum": float(loss.double().sum() + grad.double().abs().sum())}
    print(json.dumps(res))


def regression(parent_lib, rounds=4):
    """v2_fwd_bwd (loss + grad) through the parent's library and through the product library."""
    libs = {"parent": str(Path(parent_lib).resolve()),
            "product": str(ROOT / "ssnt-tts-rust_amd" / "lib" / "libssnt_tts_c.so")}
    res = {k: [] for k in libs}
    for r in range(rounds):
        for name in (list(libs) if r % 2 == 0 else list(libs)[::-1]):
            out = subprocess.run([sys.executable, __file__, "--f4-child", libs[name]], capture_output=True,
                                 text=True, timeout=300, env=dict(os.environ))
            if out.returncode != 0:
                raise RuntimeError(out.stderr[-800:])
            res[name].append(json.loads(out.stdout.strip().splitlines()[-1]))
    row = {"workload": f"v2_fwd_bwd B={B} I={I} O={O} D={D}, parent commit against this tree", "rounds": rounds}
    for mode in ("band", "test"):
        for name, rs in res.items():
            us = sorted(x[mode]["us"] for x in rs)
            row[f"{mode}_{name}_us"] = {"median": float(np.median(us)), "min": us[0], "max": us[-1]}
        row[f"{mode}_same_checksum"] = len({x[mode]["checksum"] for rs in res.values() for x in rs}) == 1
    return row


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
    ap.add_argument("--parent-lib", type=Path, default=None, help="a build of the parent commit's library")
    ap.add_argument("--f4-child", type=str, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", type=Path, default=None, help="JSON-lines file to (over)write")
    a = ap.parse_args()
    if a.f4_child:
        f4_child(a.f4_child)
    elif a.accuracy:
        accuracy(a.out or OUT_ACC)
    else:
        timing(a.out or OUT, a.parent_lib)


if __name__ == "__main__":
    main()
