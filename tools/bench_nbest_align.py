#!/usr/bin/env python3
"""Time the exact N-best alignment beside its neighbours, in one process on one GPU:

  ssnt_nbest_align            B=256 T=200 U=80 at N = 1, 2, 4, 8 and B=64 T=2000 U=400 at N = 1, 2, 4,
                              each with paths (log_prob + position + duration) and log_prob only
  the two C entries alone     ssnt_nbest_align_device / ssnt_viterbi_align_device with paths: one launch
                              per call, without the mirror's status reset and `count`
  ssnt_viterbi_align          the same two shapes (rank 0 of every N)
  ssnt_fwd_bwd(need_grad)     the same two shapes
  lattice_beam_search_decode  W=4 at the first shape (the pruned search the N-best is exact for)

GPU time as tools/bench_viterbi.py: HIP events around `iters` back-to-back calls, median of 5
rounds. One JSON line per shape and N, also written to profiles/nbest_align.jsonl with the source
hash bench.py's roofline uses. `ratio_to_viterbi` divides by ssnt_viterbi_align of the same run."""
import ctypes
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
OUT = ROOT / "profiles" / "nbest_align.jsonl"


def shape(B, T, U, ns, iters, decode_w=None):
    lt = torch.from_numpy(O.synth_log_trans(B, T, U, seed=0)).to(DEV)
    sl = torch.full((B,), T, dtype=torch.int32, device=DEV)
    pl = torch.full((B,), U, dtype=torch.int32, device=DEV)
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    vo = {"log_prob": torch.empty(B, device=DEV),
          "position": torch.empty((B, T), dtype=torch.int32, device=DEV),
          "duration": torch.empty((B, U), dtype=torch.int32, device=DEV), "status": st}
    fo = {"loss": torch.empty(B, device=DEV), "grad": torch.empty((B, T, U, 2), device=DEV), "status": st}
    S.ssnt_viterbi_align(lt, sl, pl, out=vo, check=True)
    S.ssnt_fwd_bwd(lt, sl, pl, out=fo, check=True)
    tv = gpu_time(lambda: S.ssnt_viterbi_align(lt, sl, pl, out=vo), iters)
    tvl = gpu_time(lambda: S.ssnt_viterbi_align(lt, sl, pl, need_path=False,
                                                out={"log_prob": vo["log_prob"], "status": st}), iters)
    tf = gpu_time(lambda: S.ssnt_fwd_bwd(lt, sl, pl, need_grad=True, out=fo), iters)
    # the C entries alone (one launch per call: no status reset, no `count`), with paths
    lib, stream = S.load(), ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    wv = torch.empty(max(8, int(lib.ssnt_viterbi_align_workspace_size(B, T, U))), dtype=torch.uint8, device=DEV)
    tvc = gpu_time(lambda: lib.ssnt_viterbi_align_device(
        ptr(lt), None, ptr(sl), ptr(pl), B, T, U, 1, ptr(vo["log_prob"]), ptr(vo["position"]),
        ptr(vo["duration"]), ptr(wv), wv.numel(), ptr(st), stream), iters)
    common = {"viterbi_us": tv * 1e6, "viterbi_log_prob_only_us": tvl * 1e6, "viterbi_c_entry_us": tvc * 1e6,
              "fwd_bwd_us": tf * 1e6}
    if decode_w:
        il = torch.full((B,), U, dtype=torch.int32, device=DEV)
        S.lattice_beam_search_decode(lt, il, decode_w)
        common["beam_decode_us"] = gpu_time(
            lambda: S.lattice_beam_search_decode(lt, il, decode_w, check=False), iters) * 1e6
        common["beam_decode_w"] = decode_w
    rows = []
    for N in ns:
        no = {"log_prob": torch.empty((B, N), device=DEV),
              "position": torch.empty((B, N, T), dtype=torch.int32, device=DEV),
              "duration": torch.empty((B, N, U), dtype=torch.int32, device=DEV), "status": st}
        r = S.ssnt_nbest_align(lt, sl, pl, N, out=no, check=True)
        assert torch.equal(r["log_prob"][:, 0], vo["log_prob"]) and torch.equal(r["position"][:, 0], vo["position"])
        tn = gpu_time(lambda: S.ssnt_nbest_align(lt, sl, pl, N, out=no), iters)
        tl = gpu_time(lambda: S.ssnt_nbest_align(lt, sl, pl, N, need_path=False,
                                                 out={"log_prob": no["log_prob"], "status": st}), iters)
        wn = torch.empty(max(8, int(lib.ssnt_nbest_align_workspace_size(B, T, U, N))), dtype=torch.uint8,
                         device=DEV)
        tnc = gpu_time(lambda: lib.ssnt_nbest_align_device(
            ptr(lt), None, ptr(sl), ptr(pl), B, T, U, N, 1, ptr(no["log_prob"]), ptr(no["position"]),
            ptr(no["duration"]), ptr(wn), wn.numel(), ptr(st), stream), iters)
        rows.append({"workload": f"N-best B={B} T={T} U={U} N={N} (log_prob + position + duration)",
                     "num_best": N, "nbest_us": tn * 1e6, "nbest_log_prob_only_us": tl * 1e6,
                     "nbest_c_entry_us": tnc * 1e6,
                     "ratio_to_viterbi": tn / tv, "ratio_to_viterbi_log_prob_only": tl / tvl,
                     "ratio_to_viterbi_c_entry": tnc / tvc,
                     "workspace_bytes": int(S.load().ssnt_nbest_align_workspace_size(B, T, U, N)),
                     **common, "source_sha": kernel_source_sha(), "device": torch.cuda.get_device_name(0)})
    return rows


def main():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", type=Path, default=OUT, help="JSON-lines file to (over)write")
    out = ap.parse_args().out
    rows = shape(256, 200, 80, (1, 2, 4, 8), 200, decode_w=4) + shape(64, 2000, 400, (1, 2, 4), 20)
    out.parent.mkdir(parents=True, exist_ok=True)
    with open(out, "w") as f:
        for r in rows:
            line = json.dumps(r)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
