"""Exact N best duration paths on the v2 lattice, CPU side: the numpy-f32 DP that defines the GPU's
answer (tests/v2_nbest_ref.py) against the enumeration of every admissible class
sequence -- values, paths, absent ranks, ties -- its N = 1 case against the best-path DP, the
independence of a rank from N, the ground the families stand on, and the presence of the new
entries in the header, the built libraries, the ctypes table and the package. No GPU."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import v2_nbest_ref as NR
import v2_viterbi_ref as VR

ROOT = Path(__file__).resolve().parent.parent
KINDS = ("tiny", "tie", "wide")


def _dp(kind, seed, mode, N):
    cs = NR.case(kind, seed, mode)
    return cs, NR.dp(*cs[:5], 0, *cs[5:], N)


@pytest.mark.parametrize("kind", KINDS)
def test_dp_equals_the_enumeration(kind):
    for seed, mode in NR.family(kind):
        for N in NR.NS:
            cs, r = _dp(kind, seed, mode, N)
            NR.check_against_paths(r, cs, NR.case_paths(kind, seed, mode), N)


def _path_counts(kind, pick):
    """Admissible sequences with positive probability, per utterance, of the family's cases that
    `pick` keeps."""
    out = []
    for seed, mode in NR.family(kind):
        if pick(mode):
            out += [sum(1 for v, _ in p if v > NR.NINF) for p in NR.case_paths(kind, seed, mode)]
    return np.array(out)


def test_the_families_are_not_empty_ground():
    for skip in (True, False):  # the wider band family: full lists, and some short ones
        c = _path_counts("wide", lambda m: m == skip)
        assert len(c) == 72 and (c >= 8).sum() >= 50 and ((c >= 1) & (c <= 7)).sum() >= 10, (skip, c)
    c = _path_counts("tiny", lambda m: m == "test_mode")
    assert len(c) == 72 and (c >= 8).sum() >= 50, c
    for mode in ("band", "no_skip"):  # the absent-rank ground
        c = _path_counts("tiny", lambda m: m == mode)
        assert len(c) == 72 and ((c >= 1) & (c <= 7)).sum() >= 25, (mode, c)


def test_tie_cases_repeat_a_value_among_the_eight_best():
    for seed in range(6):
        cs, r = _dp("tie", seed, True, 8)
        lp = r["log_prob"]
        rep = (lp[:, 1:] == lp[:, :-1]) & (lp[:, 1:] > -np.inf)
        assert np.all(rep.any(axis=1)), (seed, lp)


@pytest.mark.parametrize("kind", KINDS)
def test_one_best_is_the_best_path_dp(kind):
    for seed, mode in NR.family(kind):
        cs, n = _dp(kind, seed, mode, 1)
        v = VR.dp(*cs[:5], 0, *cs[5:])
        assert n["log_prob"][:, 0].tobytes() == v["log_prob"].tobytes()
        for k in ("duration_class", "duration", "total"):
            assert np.array_equal(n[k][:, 0], v[k]), (kind, seed, mode, k)
        assert np.array_equal(n["count"], (v["log_prob"] > -np.inf).astype(np.int32))


@pytest.mark.parametrize("kind", KINDS)
def test_rank_does_not_depend_on_n(kind):
    for seed, mode in NR.family(kind):
        _, big = _dp(kind, seed, mode, 8)
        for N in (1, 2, 3, 4):
            _, r = _dp(kind, seed, mode, N)
            assert r["log_prob"].tobytes() == np.ascontiguousarray(big["log_prob"][:, :N]).tobytes()
            for k in ("duration_class", "duration", "total"):
                assert np.array_equal(r[k], big[k][:, :N]), (kind, seed, mode, N, k)
            assert np.array_equal(r["count"], np.minimum(big["count"], N))


def test_infeasible_rules():
    logits = np.zeros((5, 4, 3), np.float32)
    logits[4] = -np.inf
    I, O = [4, 0, 5, 4, 4], [10, 3, 10, 13, 10]  # ok, I = 0, I > T, O > max_total, all -inf
    r = NR.dp(logits, [0, 2, 3], I, O, 12, 0, True, False, 4)
    assert r["count"].tolist() == [4, 0, 0, 0, 0]
    assert np.all(r["log_prob"][0] == 0.0) and np.all(r["total"][0] == 10)
    assert np.all(np.isneginf(r["log_prob"][1:])) and np.all(r["total"][1:] == -1)
    assert np.all(r["duration_class"][1:] == -1) and np.all(r["duration"][1:] == 0)
    r = NR.dp(logits, [0, -1, 3], I, O, 12, 0, True, False, 4)  # a negative entry: nothing feasible
    assert np.all(r["count"] == 0) and np.all(np.isneginf(r["log_prob"]))


def _header_functions():
    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "ssnt_tts_c.h").read_text(), flags=re.S)
    return dict(re.findall(r"\b([A-Za-z_]\w*)\s*\(([^;{]*)\)\s*;", re.sub(r"#.*", "", txt)))


def test_v2_nbest_surface():
    from ssnt_tts_amd._lib import SIGNATURES, load
    fns = _header_functions()
    new = (("ssnt_v2_nbest_align_workspace_size", 5), ("ssnt_v2_nbest_align_device", 20))
    for name, nargs in new:
        assert name in fns, name
        assert len(fns[name].split(",")) == nargs, name
        assert name in SIGNATURES and len(SIGNATURES[name][1]) == nargs, name
    for lib in ("lib/libssnt_tts_c.so", "lib/ab/libssnt_tts_c_ab.so"):
        path = ROOT / "ssnt-tts-rust_amd" / lib
        assert path.exists(), f"build the library first (make): {path}"
        out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True,
                             text=True, check=True).stdout
        exported = set(line.split()[-1] for line in out.splitlines() if " T " in line)
        for name, _ in new:
            assert name in exported, (name, lib)
    q = load().ssnt_v2_nbest_align_workspace_size  # dlopen only; the size query is host arithmetic
    assert q(64, 400, 2000, False, 1) == 0  # configs[4], band mode, N = 1: the entries fit LDS
    assert q(64, 400, 2000, False, 8) >= 64 * 400 * 308 * 8  # ... and 8 per cell do not
    assert q(0, 400, 2000, True, 4) == 0 and q(64, 400, 2000, True, 0) == 0 and q(64, 400, 2000, True, 9) == 0
    big = q(64, 400, 2000, True, 4)         # test mode: 400 rows of 4 * 2001 bytes do not
    assert big >= 64 * 400 * 2001 * 4 and big % 16 == 0
    assert q(64, 400, 2000, True, 3) == big  # N = 3 runs at list width 4
    import ssnt_tts_amd
    assert "v2_nbest_align" in ssnt_tts_amd.__all__ and callable(ssnt_tts_amd.v2_nbest_align)
