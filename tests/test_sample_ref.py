"""The float64 sampling reference (tests/sample_ref.py) on the CPU: its path
frequencies against the brute-force posterior, the sequential f32 path sum, the clamp, and the share
of unclear samples in the cases the GPU test uses (tests/sample_cases.py)."""
import numpy as np
import pytest

import sample_cases as SC
import sample_ref as SR


@pytest.mark.parametrize("terminal", [False, True])
@pytest.mark.parametrize("obs", [False, True])
def test_frequencies_match_the_brute_force_posterior(obs, terminal):
    # every (S,P) of T <= 7, U <= 4; 8192 draws each, fixed seeds; within 5 binomial standard
    # deviations on every path with posterior >= 1e-3 (a scratch run's maximum was 2.4). The terminal
    # emit is common to all paths of an utterance: it changes log_prob, not the distribution
    T, U, N = 7, 4, 8192
    worst = 0.0
    for S in range(1, T + 1):
        for P in range(1, min(S, U) + 1):
            lt, lo = SC.lattice(1, T, U, 100 * S + 10 * P + 2 * obs + terminal, obs)
            lt, lo = lt[0], None if lo is None else lo[0]
            u = np.random.default_rng(7 * S + P).random((N, T), dtype=np.float32)
            r = SR.sample(lt, S, P, u, lo)
            assert r["feasible"]
            post = SR.path_posterior(lt, S, P, lo)
            assert abs(sum(post.values()) - 1) < 1e-12
            worst = max(worst, SR.frequency_deviation(r["position"], S, post))
            # log_prob of a drawn path: the f32 sum agrees with the float64 score
            pos = r["position"][0]
            v = SR.path_log_prob_f32(lt, lo, pos, terminal)
            la, _, _ = SR.log_alpha(lt, S, P, lo)
            logz = la[S - 1, P - 1]
            q = post[tuple(int(x) for x in pos[:S])]
            want = np.log(q) + logz + (float(lt[S - 1, P - 1, 0]) if terminal else 0.0)
            assert abs(float(v) - want) < 1e-4
    print("largest deviation in sigma:", worst)
    assert worst <= 5.0


def test_gpu_frequency_case_passes_on_the_reference():
    c = SC.frequency()
    post = SR.path_posterior(c["lt"][0], 7, 3, c["lo"][0])
    assert len(post) == 15
    dev = SR.frequency_deviation(c["ref"]["position"].reshape(-1, 7), 7, post)
    print("deviation in sigma:", dev)
    assert dev <= 5.0


def test_clamp_and_forced_decisions():
    u = np.array([1.0, np.nan, -1.0, 0.5, 2.0, -0.0], np.float32)
    c = SR.clamp_uniform(u)
    assert c.dtype == np.float32
    assert c[0] == SR.U_MAX and c[1] == 0 and c[2] == 0 and c[3] == 0.5 and c[4] == SR.U_MAX and c[5] == 0
    assert float(SR.U_MAX) == 1 - 2.0 ** -24
    # S == P: every move is forced, whatever u says
    lt, _ = SC.lattice(1, 6, 6, 3)
    for val in (0.0, 1.0, np.nan):
        r = SR.sample(lt[0], 6, 6, np.full((2, 6), val, np.float32))
        assert r["feasible"] and np.array_equal(r["position"][0], np.arange(6))
        assert np.all(np.isinf(r["margin"]))  # forced decisions carry no margin
    # P == 1: every stay is forced
    r = SR.sample(lt[0], 6, 1, np.zeros((1, 6), np.float32))
    assert np.array_equal(r["position"][0], np.zeros(6)) and r["duration"][0, 0] == 6


def test_infeasible_rule():
    lt, _ = SC.lattice(1, 6, 4, 5)
    u = np.full((2, 6), 0.5, np.float32)
    for S, P in [(0, 1), (3, 0), (2, 3), (7, 2), (3, 5)]:
        r = SR.sample(lt[0], S, P, u)
        assert not r["feasible"] and np.all(r["position"] == -1) and np.all(r["duration"] == 0)
    dead = lt[0].copy()
    dead[2] = -np.inf
    r = SR.sample(dead, 6, 3, u)
    assert not r["feasible"]


def test_unclear_share_of_the_gpu_cases():
    # the cap the GPU test relies on: <= 25 % unclear in every case, <= 5 % over all of them
    from ssnt_tts_amd._lib import load
    lib = load()  # dlopen only; the size query is host code
    unclear = total = 0
    for name, c in SC.capped(lib):
        n, t = SC.unclear_share(c)
        print(f"{name}: {n} of {t} unclear")
        assert t >= 1 and n <= SC.CAP_CASE * t, name
        unclear, total = unclear + n, total + t
    for K in SC.K_EDGES:  # (the K = 1 and 2 cases have fewer than 32 samples: none may be unclear)
        if 4 * K < 32:
            assert SC.unclear_share(SC.k_edge(K))[0] == 0, K
    print(f"all: {unclear} of {total} unclear")
    assert unclear <= SC.CAP_ALL * total
    # the exponent-range case is outside the cap but must leave something to compare
    n, t = SC.unclear_share(SC.exponent_range())
    print(f"exponent range: {n} of {t} unclear")
    assert n < t


# The LDS-to-workspace switch of the size query, from the library before the scaffold was shared
# (csrc/align_dev.h): per number of samples, the largest T with a zero answer for each U, and the
# bytes at T + 1 with B = 3.
SWITCH_U = (1, 64, 65, 128, 129, 256, 257, 512, 513, 1024)
SWITCH = {
    1: ((1520, 1362, 2226, 2147, 306, 226, 753, 673, 368, 289),
        (36504, 32712, 106896, 103104, 29472, 21792, 144768, 129408, 141696, 111360)),
    2: ((760, 681, 1113, 1073, 153, 113, 120, 80, 56, 16),
        (36528, 32736, 106944, 103104, 29568, 21888, 46464, 31104, 43776, 13056)),
    16: ((95, 85, 139, 134, 19, 14, 15, 10, 7, 2),
         (36864, 33024, 107520, 103680, 30720, 23040, 49152, 33792, 49152, 18432)),
    64: ((23, 21, 34, 33, 4, 3, 3, 2, 1, 0),
         (36864, 33792, 107520, 104448, 30720, 24576, 49152, 36864, 49152, 24576)),
}


@pytest.mark.parametrize("NS", sorted(SWITCH))
def test_workspace_switch_points_are_pinned(NS):
    from test_viterbi_ref import last_zero_T
    from ssnt_tts_amd._lib import load
    q = load().ssnt_sample_align_workspace_size  # dlopen only; the size query is host code
    for U, T, nbytes in zip(SWITCH_U, *SWITCH[NS]):
        assert last_zero_T(lambda t: q(3, t, U, NS)) == T, U
        assert (T == 0 or q(3, T, U, NS) == 0) and q(3, T + 1, U, NS) == nbytes, U
