"""The definition of the banded best path on the CPU: the band-coordinate
recurrence of tests/band_viterbi_ref.py has the bits and the path of viterbi_ref.dp on
band_ref.embed of the band, and both agree with a brute force over the paths inside the band."""
import numpy as np
import pytest

import band_ref as BR
import band_viterbi_ref as BV
import viterbi_ref as VR
from contract_cases import same_bits


def _by_definition(c, terminal=True):
    """viterbi_ref.dp on the embedding; duration cut or padded to max(P) columns."""
    lt, lo = BR.embed(c["lt"], c["lo"], c["bs"], c["S"], c["P"])
    o = VR.dp(lt, c["S"], c["P"], lo, terminal)
    U = int(max(1, c["P"].max()))
    dur = np.zeros((len(c["S"]), U), np.int32)
    n = min(U, o["duration"].shape[1])
    dur[:, :n] = o["duration"][:, :n]
    assert not o["duration"][:, n:].any()
    return {"log_prob": o["log_prob"], "position": o["position"], "duration": dur}


def _assert_equal(r, o, what):
    assert same_bits(r["log_prob"], o["log_prob"]), (what, r["log_prob"], o["log_prob"])
    assert np.array_equal(r["position"], o["position"]), what
    assert np.array_equal(r["duration"], o["duration"]), what


@pytest.mark.parametrize("obs", [False, True], ids=["obs0", "obs1"])
@pytest.mark.parametrize("R", BV.WIDTHS)
def test_band_recurrence_is_dp_on_the_embedding(R, obs):
    c = BV.case(R, obs)
    for terminal in (True, False):
        r = BV.dp(c["lt"], c["lo"], c["bs"], c["S"], c["P"], terminal)
        _assert_equal(r, _by_definition(c, terminal), (R, obs, terminal))
        assert np.isfinite(r["log_prob"]).all()
        for b in range(len(c["S"])):
            S, pos = int(c["S"][b]), r["position"][b]
            assert np.all((c["bs"][b, :S] <= pos[:S]) & (pos[:S] < c["bs"][b, :S] + R))


def test_tie_rich_inputs():
    feasible = total = ties = 0
    for R in BV.WIDTHS:
        for obs in (False, True):
            c = BV.tie_case(R, obs)
            o = _by_definition(c)
            _assert_equal(BV.dp(c["lt"], c["lo"], c["bs"], c["S"], c["P"]), o, (R, obs))
            feasible += int(np.sum(o["log_prob"] > -np.inf))
            total += len(c["S"])
            ties += int(np.sum(c["lt"][..., 0] == c["lt"][..., 1]))
    assert BV.TIE_NINF_SHARE <= 0.01
    assert total == 280 and feasible >= 0.75 * total, (feasible, total)  # by the reference alone
    assert feasible < total  # (and some utterance has no path left)
    assert ties > 0


def test_brute_force_over_every_small_band():
    rng = np.random.default_rng(0)
    n = 0
    for T in range(1, 8):
        for R in (1, 2, 3):
            for S in range(1, T + 1):
                for P in range(1, S + 1):
                    for bs in BV.all_valid_bands(T, S, P, R):
                        kind = n % 3
                        if kind == 0:    # random reals
                            lt = (rng.standard_normal((T, R, 2)) * 3).astype(np.float32)
                        elif kind == 1:  # small integers: ties
                            lt = -rng.integers(0, 3, size=(T, R, 2)).astype(np.float32)
                        else:            # some -inf
                            lt = (rng.standard_normal((T, R, 2)) * 3).astype(np.float32)
                            lt[rng.random(lt.shape) < 0.15] = -np.inf
                        lo = (rng.standard_normal((T, R)) * 5).astype(np.float32) if n % 2 else None
                        term = n % 4 < 2
                        best, arg = BV.brute_force(lt, lo, bs, S, P, term)
                        v, pos = BV.dp_one(lt, lo, bs, S, P, term)
                        assert same_bits(np.float32(v), np.float32(best)), (T, R, S, P, bs)
                        if pos is None:
                            assert not arg
                        else:
                            assert tuple(int(x) for x in pos) in arg, (T, R, S, P, bs)
                        n += 1
    assert n > 800  # (the loops are not empty: 884 bands at S in {T, T-2} alone)


def test_infeasible_and_refused_utterances():
    R, T = 4, 12
    rng = np.random.default_rng(2)
    #      ok      S<P     S=0     P=0     S>T      ok, but P > max_pos
    SP = [(12, 6), (3, 5), (0, 2), (4, 0), (13, 3), (10, 9)]
    S = np.array([s for s, _ in SP], np.int32)
    P = np.array([p for _, p in SP], np.int32)
    bs = np.zeros((len(SP), T), np.int32)
    bs[0] = BR.make_band("random", T, 12, 6, R, rng)
    bs[5] = BR.make_band("random", T, 10, 9, R, rng)
    lt, lo = BV.synth(len(SP), T, R, True, 4)
    r = BV.dp(lt, lo, bs, S, P, max_pos=8)
    assert np.isfinite(r["log_prob"][0]) and r["duration"][0].sum() == 12
    for b in range(1, len(SP)):
        assert r["log_prob"][b] == -np.inf and np.all(r["position"][b] == -1) and not r["duration"][b].any()
    bad = bs.copy()
    bad[0, 3:] += 2
    assert BV.dp(lt, lo, bad, S, P)["log_prob"][0] == -np.inf
