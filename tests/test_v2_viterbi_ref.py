"""Best duration path on the v2 lattice, CPU side: the numpy-f32 DP that defines the GPU's answer
(tests/v2_viterbi_ref.py) against brute force over every class sequence, a tie-rich set, and the
presence of the new C-ABI entries in the header, the built library and the ctypes table. No GPU."""
import re
import subprocess
from pathlib import Path

import numpy as np
import v2_viterbi_ref as VR

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ["ssnt_v2_viterbi_align_workspace_size", "ssnt_v2_viterbi_align_device"]


def test_dp_equals_brute_force():
    feasible = tied = 0
    for seed in range(6):
        for mode in VR.MODES:
            case = VR.tiny_case(seed, mode)
            f, t = VR.check_against_brute_force(VR.dp(*case[:5], 0, *case[5:]), case,
                                                VR.case_brute_force("tiny", seed, mode))
            feasible += f
            tied += t
    # 216 utterances; half of them feasible at the least, so the test cannot pass on empty
    # lattices (a prototype counted 150, none of them tied: every path above was THE path)
    assert feasible >= 108, feasible


def test_dp_tie_rich():
    feasible = tied = 0
    for seed in range(6):
        for test_mode in (False, True):
            case = VR.tie_case(seed, test_mode)
            f, t = VR.check_against_brute_force(VR.dp(*case[:5], 0, *case[5:]), case,
                                                VR.case_brute_force("tie", seed, test_mode))
            feasible += f
            tied += t
    assert tied >= 12, (feasible, tied)  # a tenth of the 120 at the least: the set is tie-rich


def test_dp_tie_keeps_the_lower_class_and_total():
    # all-equal logits: every admissible sequence ties. I=3, O=6 admits only durations 2, 2, 2
    # (band rows [1,2], [3,4], {6}); classes 2 and 3 both add 2: the lower wins
    logits = np.full((1, 3, 4), -1.0, np.float32)
    r = VR.dp(logits, [0, 1, 2, 2], [3], [6], 6, 0, True, False)
    assert r["log_prob"][0] == np.float32(-3.0) and r["total"][0] == 6
    assert r["duration_class"][0].tolist() == [2, 2, 2] and r["duration"][0].tolist() == [2, 2, 2]
    # test mode: the final total is free; every total ties, the lowest (all class 0) wins
    r = VR.dp(logits, [0, 1, 2, 2], [3], [6], 6, 0, True, True)
    assert r["total"][0] == 0 and r["duration_class"][0].tolist() == [0, 0, 0]


def test_dp_infeasible_rules():
    logits = np.zeros((5, 4, 3), np.float32)
    logits[4] = -np.inf
    I, O = [4, 0, 5, 4, 4], [10, 3, 10, 13, 10]  # ok, I = 0, I > T, O > max_total, all -inf
    r = VR.dp(logits, [0, 2, 3], I, O, 12, 0, True, False)
    assert r["log_prob"][0] == 0.0 and r["total"][0] == 10 and r["duration"][0].sum() == 10
    assert np.all(np.isneginf(r["log_prob"][1:])) and np.all(r["total"][1:] == -1)
    assert np.all(r["duration_class"][1:] == -1) and np.all(r["duration"][1:] == 0)
    r = VR.dp(logits, [0, -1, 3], I, O, 12, 0, True, False)  # a negative entry: nothing feasible
    assert np.all(np.isneginf(r["log_prob"])) and np.all(r["total"] == -1)


def _header_functions():
    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "ssnt_tts_c.h").read_text(), flags=re.S)
    return set(re.findall(r"\b([A-Za-z_]\w*)\s*\([^;{]*\)\s*;", re.sub(r"#.*", "", txt)))


def test_v2_viterbi_entries_in_header_library_and_ctypes_table():
    from ssnt_tts_amd._lib import SIGNATURES, load
    fns = _header_functions()
    for lib in ("lib/libssnt_tts_c.so", "lib/ab/libssnt_tts_c_ab.so"):
        path = ROOT / "ssnt-tts-rust_amd" / lib
        assert path.exists(), f"build the library first (make): {path}"
        out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True,
                             text=True, check=True).stdout
        exported = set(line.split()[-1] for line in out.splitlines() if " T " in line)
        for s in NEW_SYMBOLS:
            assert s in exported, (s, lib)
    for s in NEW_SYMBOLS:
        assert s in fns and s in SIGNATURES, s
    lib = load()  # dlopen only; the size query is host arithmetic
    q = lib.ssnt_v2_viterbi_align_workspace_size
    assert q(64, 400, 2000, False) == 0  # configs[4], band mode: the backpointers fit LDS
    assert q(0, 400, 2000, True) == 0
    big = q(64, 400, 2000, True)         # test mode: 400 rows of 2001 bytes do not
    assert big >= 64 * 400 * 2001 and big % 16 == 0
    import ssnt_tts_amd
    assert "v2_viterbi_align" in ssnt_tts_amd.__all__
