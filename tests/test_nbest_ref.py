"""Exact N-best alignments, CPU side: the numpy-f32 DP that defines the GPU's answer
(tests/nbest_ref.py) against brute force over every monotone path -- values, paths,
absent ranks, ties -- its N = 1 case against the best-path DP, and the presence of the new entries
in the header, the ctypes table and the package. No GPU."""
import re
from pathlib import Path

import numpy as np
import pytest

import nbest_ref as NR
import viterbi_ref as VR

ROOT = Path(__file__).resolve().parent.parent
T, U = 8, 5
SP = [(S, P) for S in range(0, T + 1) for P in range(0, U + 1)]
NS = (1, 2, 3, 4, 8)
KINDS = ("random", "tie_rich", "zeros")


def _lattice(kind, obs):
    rng = np.random.default_rng(17 + 3 * KINDS.index(kind) + obs)
    if kind == "tie_rich":
        lt = rng.choice(np.array([-0.5, -1.0, -1.5], np.float32), size=(T, U, 2))
        lo = rng.choice(np.array([-0.5, -1.0, -1.5], np.float32), size=(T, U)) if obs else None
    else:
        lt = np.log(rng.uniform(0.05, 1.0, size=(T, U, 2))).astype(np.float32)
        lo = (rng.standard_normal((T, U)) * 3 - 2).astype(np.float32) if obs else None
        if kind == "zeros":
            lt[rng.random((T, U, 2)) < 0.2] = -np.inf
    return lt, lo


_BRUTE = {}


def _brute(kind, obs, terminal):
    """Brute force of every (S, P), once per lattice: it does not depend on N."""
    key = (kind, obs, terminal)
    if key not in _BRUTE:
        lt, lo = _lattice(kind, obs)
        _BRUTE[key] = [NR.brute_force(lt, S, P, lo, terminal) for S, P in SP]
    return _BRUTE[key]


def _check(kind, obs, terminal, N):
    """dp against brute force on every (S, P); returns (cases, cases with a tie inside the top N)."""
    lt, lo = _lattice(kind, obs)
    B = len(SP)
    r = NR.dp(np.broadcast_to(lt, (B,) + lt.shape), [s for s, _ in SP], [p for _, p in SP], N,
              None if lo is None else np.broadcast_to(lo, (B,) + lo.shape), terminal)
    ties = 0
    for b, ((S, P), paths) in enumerate(zip(SP, _brute(kind, obs, terminal))):
        where = (kind, obs, terminal, N, S, P)
        top = NR.top_values(paths, N)
        assert r["log_prob"][b].tobytes() == top.tobytes(), where
        finite = sum(1 for v, _ in paths if v > NR.NINF)
        n = min(N, finite)
        assert r["count"][b] == n, where  # absent ranks exactly beyond min(N, finite paths)
        assert np.all(np.isneginf(r["log_prob"][b, n:])), where
        assert np.all(r["position"][b, n:] == -1) and np.all(r["duration"][b, n:] == 0), where
        value_of = {path: v for v, path in paths}
        seen = set()
        for k in range(n):
            path = tuple(r["position"][b, k, :S].tolist())
            assert path not in seen, where  # distinct
            seen.add(path)
            assert np.float32(value_of[path]).tobytes() == r["log_prob"][b, k].tobytes(), where
            assert np.all(r["position"][b, k, S:] == -1), where
            assert np.array_equal(np.bincount(path, minlength=U), r["duration"][b, k]), where
        ties += int(n > 1 and np.any(top[1:n] == top[:n - 1]))
    return len(SP), ties


@pytest.mark.parametrize("terminal", [True, False])
@pytest.mark.parametrize("obs", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_dp_equals_brute_force(kind, obs, terminal):
    for N in NS:
        cases, _ = _check(kind, obs, terminal, N)
        assert cases == len(SP)


def test_tie_rich_lattices_have_ties_inside_the_top_n():
    # Values are sums of at most 8 (16 with log_obs) terms from {-0.5, -1, -1.5}: at most 33
    # distinct sums for up to 35 paths per cell, so ties among the best N > 1 are common. The floor
    # is a tenth of the (S, P, N > 1) cases that have at least two paths (S > P >= 2 or so).
    total = ties = 0
    for obs in (False, True):
        for terminal in (True, False):
            for N in NS:
                c, t = _check("tie_rich", obs, terminal, N)
                total, ties = total + c, ties + t
    assert total == 4 * len(NS) * len(SP)
    assert ties >= 60, ties


@pytest.mark.parametrize("obs", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_one_best_is_the_best_path_dp(kind, obs):
    lt, lo = _lattice(kind, obs)
    B = len(SP)
    ltb = np.broadcast_to(lt, (B,) + lt.shape)
    lob = None if lo is None else np.broadcast_to(lo, (B,) + lo.shape)
    S, P = [s for s, _ in SP], [p for _, p in SP]
    for terminal in (True, False):
        n = NR.dp(ltb, S, P, 1, lob, terminal)
        v = VR.dp(ltb, S, P, lob, terminal)
        assert n["log_prob"][:, 0].tobytes() == v["log_prob"].tobytes()
        assert np.array_equal(n["position"][:, 0], v["position"])
        assert np.array_equal(n["duration"][:, 0], v["duration"])
        assert np.array_equal(n["count"], (v["log_prob"] > -np.inf).astype(np.int32))


def test_rank_does_not_depend_on_n():
    lt, lo = _lattice("tie_rich", True)
    B = len(SP)
    ltb = np.broadcast_to(lt, (B,) + lt.shape)
    lob = np.broadcast_to(lo, (B,) + lo.shape)
    S, P = [s for s, _ in SP], [p for _, p in SP]
    big = NR.dp(ltb, S, P, 8, lob)
    for N in (1, 2, 3, 4):
        r = NR.dp(ltb, S, P, N, lob)
        for k in ("log_prob", "position", "duration"):
            assert np.array_equal(r[k], big[k][:, :N]), (N, k)


def _header_functions():
    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "ssnt_tts_c.h").read_text(), flags=re.S)
    return dict(re.findall(r"\b([A-Za-z_]\w*)\s*\(([^;{]*)\)\s*;", re.sub(r"#.*", "", txt)))


def test_nbest_surface():
    from ssnt_tts_amd._lib import SIGNATURES
    fns = _header_functions()
    for name, nargs in (("ssnt_nbest_align_workspace_size", 4), ("ssnt_nbest_align_device", 16)):
        assert name in fns, name
        assert len(fns[name].split(",")) == nargs, name
        assert name in SIGNATURES and len(SIGNATURES[name][1]) == nargs, name
    import ssnt_tts_amd
    assert "ssnt_nbest_align" in ssnt_tts_amd.__all__ and callable(ssnt_tts_amd.ssnt_nbest_align)
