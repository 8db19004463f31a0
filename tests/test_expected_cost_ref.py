"""The float64 reference of the expected path cost (tests/expected_cost_ref.py)
against brute-force path enumeration and against torch's double backward, plus the identities and
closed forms the GPU tests lean on. CPU only."""
import numpy as np
import pytest

import expected_cost_ref as R

KEYS = ("grad_trans", "grad_cost", "grad_obs")


def _case(seed, T, U, obs, ninf_frac=0.0):
    rng = np.random.default_rng(seed)
    lt = np.log(rng.dirichlet([1.5, 1.0], size=(T, U)))
    if ninf_frac:
        lt = np.where(rng.random((T, U, 2)) < ninf_frac, -np.inf, lt)
    lo = rng.normal(0, 1, (T, U)) if obs else None
    cost = rng.normal(0, 1, (T, U, 2))
    return lt, cost, lo


# (S, P, T, U): ragged S < T, P = 1, S = P, one step
SHAPES = [(7, 4, 9, 5), (5, 1, 5, 3), (4, 4, 6, 4), (1, 1, 2, 2), (11, 3, 11, 3), (6, 5, 7, 6)]


@pytest.mark.parametrize("obs", [False, True])
@pytest.mark.parametrize("terminal", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_dp_matches_brute_force(shape, terminal, obs):
    S, P, T, U = shape
    lt, cost, lo = _case(S * 31 + P, T, U, obs)
    d = R.expected_cost(lt, cost, S, P, lo, terminal)
    bf = R.brute_force(lt, cost, S, P, lo, terminal)
    assert d["feasible"]
    assert abs(d["risk"] - bf["risk"]) < 1e-12
    assert abs(d["loss"] - bf["loss"]) < 1e-12
    for k in KEYS:
        assert np.abs(d[k] - bf[k]).max() < 1e-12, k


def test_dp_matches_brute_force_with_blocked_edges():
    for seed in range(6):
        lt, cost, lo = _case(seed, 8, 4, True, ninf_frac=0.2)
        d = R.expected_cost(lt, cost, 8, 4, lo, True)
        if not d["feasible"]:
            continue
        bf = R.brute_force(lt, cost, 8, 4, lo, True)
        assert abs(d["risk"] - bf["risk"]) < 1e-12
        for k in KEYS:
            assert np.abs(d[k] - bf[k]).max() < 1e-12, (seed, k)


@pytest.mark.parametrize("obs,terminal,shape", [(False, True, (6, 3, 7, 4)), (True, True, (6, 3, 7, 4)),
                                                (True, False, (5, 4, 5, 4)), (False, False, (7, 2, 8, 3)),
                                                (True, True, (4, 1, 4, 2))])
def test_dp_matches_torch_double_backward(obs, terminal, shape):
    S, P, T, U = shape
    lt, cost, lo = _case(S + 100 * P, T, U, obs)
    d = R.expected_cost(lt, cost, S, P, lo, terminal)
    t = R.torch_double_backward(lt, cost, S, P, lo, terminal)
    assert abs(d["risk"] - t["risk"]) < 1e-13
    assert abs(d["loss"] - t["loss"]) < 1e-13
    live = R.live_edges(lt.shape, S, P, terminal)
    for k in ("grad_trans", "grad_cost"):
        assert np.abs(d[k] - np.where(live, t[k], 0.0)).max() < 1e-13, k
    if obs:
        assert np.abs(d["grad_obs"][:S, :P] - t["grad_obs"][:S, :P]).max() < 1e-13


@pytest.mark.parametrize("obs", [False, True])
def test_identities(obs):
    S, P, T, U = 40, 13, 44, 16
    lt, cost, lo = _case(5, T, U, obs)
    d = R.expected_cost(lt, cost, S, P, lo, True)
    assert np.abs(d["grad_trans"][:S - 1].sum(axis=(1, 2))).max() < 1e-12
    assert np.abs(d["grad_cost"][:S - 1].sum(axis=(1, 2)) - 1.0).max() < 1e-12
    assert d["grad_cost"][S - 1, P - 1, 0] == 1.0 and d["grad_trans"][S - 1].max() == 0.0
    assert np.all(d["grad_trans"][S:] == 0) and np.all(d["grad_cost"][:, P:] == 0)


@pytest.mark.parametrize("obs", [False, True])
@pytest.mark.parametrize("terminal", [False, True])
def test_entropy_matches_brute_force(terminal, obs):
    S, P, T, U = 9, 4, 10, 5
    lt, _, lo = _case(77, T, U, obs)
    c = R.entropy_cost(lt, S, lo)
    d = R.expected_cost(lt, c, S, P, lo, terminal)
    bf = R.brute_force(lt, c, S, P, lo, terminal)
    h = -d["loss"] - d["risk"] - (lo[0, 0] if obs else 0.0)
    assert abs(h - bf["entropy"]) < 1e-12


def test_zero_cost_is_exactly_zero():
    lt, cost, lo = _case(3, 12, 6, True)
    d = R.expected_cost(lt, np.zeros_like(cost), 12, 5, lo, True)
    assert d["risk"] == 0.0
    assert not d["grad_trans"].any() and not d["grad_obs"].any()


@pytest.mark.parametrize("terminal", [False, True])
def test_constant_cost(terminal):
    S, P, T, U = 17, 6, 17, 7
    lt, cost, lo = _case(9, T, U, True)
    d = R.expected_cost(lt, np.full_like(cost, 2.5), S, P, lo, terminal)
    assert abs(d["risk"] - 2.5 * (S - 1 + terminal)) < 1e-12
    assert np.abs(d["grad_trans"]).max() < 1e-12 and np.abs(d["grad_obs"]).max() < 1e-12


def test_infeasible_rule_and_scale():
    lt, cost, lo = _case(1, 6, 4, True)
    for S, P in [(2, 3), (0, 1), (3, 0), (7, 2), (3, 5)]:
        d = R.expected_cost(lt, cost, S, P, lo, True)
        assert not d["feasible"] and d["risk"] == 0.0 and d["loss"] == np.inf
        assert not d["grad_trans"].any() and not d["grad_cost"].any() and not d["grad_obs"].any()
    blocked = lt.copy()
    blocked[2, :, 1] = -np.inf  # no shift at step 2, and P - 1 shifts needed in S - 1 = 3 steps
    blocked[0, :, 0] = -np.inf
    assert not R.expected_cost(blocked, cost, 4, 4, lo, True)["feasible"]
    c = np.zeros((6, 4, 2))
    c[1, 0, 0], c[1, 3, 1], c[4, 1, 0], c[5, 3, 0] = -3.0, 100.0, 2.0, 7.0
    assert R.scale(c, 6, 4, True) == 3.0 + 2.0 + 7.0     # (1,3,1) is the masked shift out of P-1
    assert R.scale(c, 6, 4, False) == 5.0
    assert R.scale(np.zeros((6, 4, 2)), 6, 4, True) == 1.0


def test_value_cases_keep_the_reference_well_defined():
    # the input value classes the GPU test adds (tests/expected_cost_cases.py `value`): the float64
    # log-domain DP is feasible and finite on each, keeps both identities, and its normaliser is the
    # one of the tame distribution (`scale` is a function of the costs and the extents only)
    import expected_cost_cases as EC
    tame = EC.reference(EC.make(4, 48, 20, 48, obs=False, S=EC.value("peaked30")["S"], P=[20, 13, 7, 12]))
    for name in EC.VALUE_NAMES:
        assert name in EC.case_makers(lambda U, obs: 8)
        c = EC.value(name[len("value-"):])
        r = EC.reference(c)
        assert r["feasible"].all() and np.array_equal(r["scale"], tame["scale"]), name
        for k in ("risk", "loss", "grad_trans", "grad_cost"):
            assert np.isfinite(r[k]).all(), (name, k)
        for b, S in enumerate(c["S"]):
            assert np.abs(r["grad_cost"][b, :S - 1].sum(axis=(1, 2)) - 1.0).max() < 1e-9, name
            assert np.abs(r["grad_trans"][b, :S - 1].sum(axis=(1, 2))).max() < 1e-9 * r["scale"][b], name


def test_underflow_safe():
    S, P, T, U = 300, 40, 300, 40
    lt, cost, lo = _case(11, T, U, False)
    d = R.expected_cost(lt - 80.0, cost, S, P, None, True)
    e = R.expected_cost(lt, cost, S, P, None, True)
    assert np.isfinite(d["loss"]) and abs(d["risk"] - e["risk"]) < 1e-9
    assert np.abs(d["grad_trans"] - e["grad_trans"]).max() < 1e-9
