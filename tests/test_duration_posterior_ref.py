"""The float64 reference of the duration posterior (tests/duration_posterior_ref.py, DESIGN.md
2.10) against brute-force path enumeration, and its identities: rows sum to 1, the mean duration
is the occupancy of tests/expected_cost_ref.py's cell posterior, impossible bins are 0. No GPU."""
import numpy as np
import pytest

import duration_posterior_cases as DC
import duration_posterior_ref as R
import expected_cost_ref as ER

SHAPES = [(S, P) for S in range(1, 8) for P in range(1, min(S, 5) + 1)]


def _inputs(S, P, obs, seed=0):
    rng = np.random.default_rng(1000 * S + 10 * P + seed)
    T, U = S + 1, P + 1  # (padding the reference must not read)
    lt = np.log(rng.dirichlet([1.5, 1.0], size=(T, U)))
    lo = 0.5 * rng.standard_normal((T, U)) if obs else None
    return lt, lo


@pytest.mark.parametrize("terminal", [False, True])
@pytest.mark.parametrize("obs", [False, True])
def test_dp_equals_brute_force(obs, terminal):
    for S, P in SHAPES:
        lt, lo = _inputs(S, P, obs)
        for D in sorted({2, 3, max(S, 2), S + 2}):
            got = R.duration_posterior(lt, S, P, D, lo, terminal)
            want = R.brute_force(lt, S, P, D, lo, terminal)
            assert got["feasible"]
            assert np.abs(got["dur_post"] - want["dur_post"]).max() <= 1e-13, (S, P, D)
            assert abs(got["loss"] - want["loss"]) <= 1e-12 * max(1.0, abs(want["loss"])), (S, P, D)


@pytest.mark.parametrize("obs", [False, True])
def test_rows_sum_to_one_and_impossible_bins_are_zero(obs):
    for S, P in SHAPES:
        lt, lo = _inputs(S, P, obs, seed=1)
        for D in (2, 3, max(S, 2), S + 2):
            dp = R.duration_posterior(lt, S, P, D, lo)["dur_post"]
            assert np.abs(dp[:P].sum(axis=1) - 1.0).max() <= 1e-13, (S, P, D)
            c = {"lt": lt[None], "S": [S], "P": [P], "D": D}
            assert not dp[DC.impossible(c)[0]].any(), (S, P, D)


@pytest.mark.parametrize("terminal", [False, True])
@pytest.mark.parametrize("obs", [False, True])
def test_mean_duration_is_the_occupancy(obs, terminal):
    for S, P in SHAPES:
        lt, lo = _inputs(S, P, obs, seed=2)
        D = S - P + 3  # D-1 >= S-P+1: every duration has its own bin
        dp = R.duration_posterior(lt, S, P, D, lo, terminal)["dur_post"]
        mean = (dp[:P] * np.arange(D)).sum(axis=1)
        assert np.abs(mean - R.occupancy(lt, S, P, lo, terminal)).max() <= 1e-12, (S, P)
        # the same occupancy from the reference of the expected cost: the posterior of entering
        # (s, p) by either edge, plus the start cell
        T, U = lt.shape[:2]
        gc = ER.expected_cost(lt, np.zeros((T, U, 2)), S, P, lo, terminal)["grad_cost"]
        occ = gc[:S - 1, :P, 0].sum(axis=0)
        occ[1:] += gc[:S - 1, :P - 1, 1].sum(axis=0)
        occ[0] += 1.0
        assert np.abs(mean - occ).max() <= 1e-12, (S, P)


def test_infeasible_and_dead_cells():
    lt, lo = _inputs(5, 3, True)
    for S, P in ((2, 3), (0, 1), (3, 0), (7, 3), (5, 5)):
        r = R.duration_posterior(lt, S, P, 4, lo)
        assert not r["feasible"] and np.isposinf(r["loss"]) and not r["dur_post"].any()
    blocked = lt.copy()
    blocked[:, 1, 1] = -np.inf  # no way out of position 1: Z = 0
    r = R.duration_posterior(blocked, 5, 3, 4, lo)
    assert not r["feasible"] and not r["dur_post"].any()
    # NaN in every cell the contract never reads changes nothing
    import contract_cases as CC
    dlt, dlo = CC.dirty_lattice(lt[None], lo[None], [5], [3], CC.VALUES["nan"], True)
    a = R.duration_posterior(lt.astype(np.float32), 5, 3, 4, lo.astype(np.float32))
    b = R.duration_posterior(dlt[0], 5, 3, 4, dlo[0])
    assert np.array_equal(a["dur_post"], b["dur_post"]) and a["loss"] == b["loss"]


def test_single_path_case_is_one_hot():
    c, dur = DC.single_path(True)
    ref = DC.reference(c)
    B, U, D = ref["dur_post"].shape
    want = np.zeros((B, U, D))
    for b in range(B):
        for p in range(int(c["P"][b])):
            want[b, p, min(dur[b, p], D - 1)] = 1.0
    assert np.abs(ref["dur_post"] - want).max() <= 1e-13
    assert not ref["dur_post"][want == 0].any()
