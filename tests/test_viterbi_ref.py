"""Best-path (Viterbi) alignment, CPU side: the numpy-f32 DP that defines the GPU's answer
(tests/viterbi_ref.py) against brute force over every monotone path, and the presence of the
new C-ABI entries in the header, the built library and the ctypes table. No GPU."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import viterbi_ref as VR

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ["ssnt_viterbi_align_workspace_size", "ssnt_viterbi_align_device"]


def _lattice(T, U, seed, obs):
    rng = np.random.default_rng(seed)
    lt = np.log(rng.uniform(0.05, 1.0, size=(T, U, 2))).astype(np.float32)
    lo = (rng.standard_normal((T, U)) * 3 - 2).astype(np.float32) if obs else None
    return lt, lo


@pytest.mark.parametrize("terminal", [True, False])
@pytest.mark.parametrize("obs", [False, True])
def test_dp_equals_brute_force_on_every_tiny_lattice(obs, terminal):
    checked = 0
    for T in range(1, 8):
        for U in range(1, 6):
            lt, lo = _lattice(T, U, 100 * T + U, obs)
            SP = [(S, P) for S in range(0, T + 1) for P in range(0, U + 1)]
            B = len(SP)
            r = VR.dp(np.broadcast_to(lt, (B,) + lt.shape),
                      [s for s, _ in SP], [p for _, p in SP],
                      None if lo is None else np.broadcast_to(lo, (B,) + lo.shape), terminal)
            for b, (S, P) in enumerate(SP):
                best, arg = VR.brute_force(lt, S, P, lo, terminal)
                assert r["log_prob"][b].tobytes() == np.float32(best).tobytes(), (T, U, S, P)
                if not arg:
                    assert np.all(r["position"][b] == -1) and np.all(r["duration"][b] == 0)
                    continue
                assert len(arg) == 1, ("tie in a fixed-seed lattice", T, U, S, P)
                assert tuple(r["position"][b, :S]) == arg[0], (T, U, S, P)
                assert np.all(r["position"][b, S:] == -1)
                assert int(r["duration"][b].sum()) == S
                assert np.all(r["duration"][b, P:] == 0)
                assert np.array_equal(np.bincount(arg[0], minlength=U), r["duration"][b])
                checked += 1
    assert checked > 200


def test_dp_tie_keeps_the_emit():
    # all-equal lattice: every path ties, so the path stays at each position as long as it can
    # going backwards from (S-1, P-1) -- i.e. it shifts as early as possible
    lt = np.full((1, 6, 3, 2), -1.0, np.float32)
    r = VR.dp(lt, [6], [3])
    assert r["position"][0].tolist() == [0, 1, 2, 2, 2, 2]
    assert r["duration"][0].tolist() == [1, 1, 4]
    assert r["log_prob"][0] == np.float32(-6.0)


def test_dp_zero_probability_and_bad_lengths():
    lt = np.log(np.full((3, 4, 2, 2), 0.5, np.float32))
    lt[0, :, 0, 1] = -np.inf  # no shift out of position 0: P = 2 unreachable
    r = VR.dp(lt, [4, 5, 4], [2, 2, 3])  # [1]: S > T, [2]: P > U
    assert np.all(np.isneginf(r["log_prob"]))
    assert np.all(r["position"] == -1) and np.all(r["duration"] == 0)


def _header_functions():
    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "ssnt_tts_c.h").read_text(), flags=re.S)
    return set(re.findall(r"\b([A-Za-z_]\w*)\s*\([^;{]*\)\s*;", re.sub(r"#.*", "", txt)))


def test_viterbi_entries_in_header_library_and_ctypes_table():
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
    assert lib.ssnt_viterbi_align_workspace_size(256, 200, 80) == 0
    assert lib.ssnt_viterbi_align_workspace_size(0, 200, 80) == 0
    big = lib.ssnt_viterbi_align_workspace_size(2, 1100, 1024)
    assert big > 0 and big % 8 == 0
    import ssnt_tts_amd
    assert "ssnt_viterbi_align" in ssnt_tts_amd.__all__


# The LDS-to-workspace switch of the size query, from the library before the scaffold was shared
# (csrc/align_dev.h): the largest T with a zero answer per U, and the bytes at T + 1 with B = 3.
SWITCH_U = (1, 64, 65, 128, 129, 256, 257, 512, 513, 1024)
SWITCH_T = (13814, 13782, 2283, 2267, 653, 1501, 846, 830, 439, 423)
SWITCH_BYTES = (331560, 330792, 109632, 108864, 62784, 144192, 162624, 159552, 168960, 162816)


def last_zero_T(query):
    """The largest T in [0, 65536) for which query(T) == 0 (0 if there is none), by bisection."""
    if query(1) > 0:
        return 0
    lo, hi = 1, 1 << 16
    assert query(hi) > 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if query(mid) == 0 else (lo, mid)
    return lo


def test_workspace_switch_points_are_pinned():
    from ssnt_tts_amd._lib import load
    q = load().ssnt_viterbi_align_workspace_size  # dlopen only; the size query is host arithmetic
    for U, T, nbytes in zip(SWITCH_U, SWITCH_T, SWITCH_BYTES):
        assert last_zero_T(lambda t: q(3, t, U)) == T, U
        assert q(3, T, U) == 0 and q(3, T + 1, U) == nbytes, U
    assert q(64, 2000, 400) == 8192000 and q(256, 200, 80) == 0
