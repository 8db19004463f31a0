"""The float64 references of the v2 expected path cost (tests/v2_expected_cost_ref.py) against each
other, on the CPU: the log-domain DP of DESIGN.md 2.9, the brute force over all D^I class sequences
and the torch double backward agree at D <= 4, I <= 6 in band mode, test mode and no-skip mode; both
identities hold; utterances without an admissible path follow the rule.

TOL: the three are float64 computations of at most 4^6 paths of 6 steps; their worst mutual
difference measured on these cases is 4e-15 (relative to the cost scale), so 1e-9 is ample."""
import numpy as np
import pytest

import v2_expected_cost_cases as C
import v2_expected_cost_ref as R

TOL = 1e-9
MODES, _tiny = C.MODES, C.tiny


def _close(a, b, sc, what):
    for k in ("risk", "loss", "grad_logits", "grad_cost"):
        d = np.max(np.abs(np.asarray(a[k], np.float64) - np.asarray(b[k], np.float64)))
        assert d <= TOL * max(sc, 1.0), (what, k, d)


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_dp_brute_force_and_double_backward_agree(seed, mode):
    tm, sk = MODES[mode]
    logits, cost, table, I, O, mt, zid, allow_skip, test_mode = _tiny(seed, tm, sk)
    feasible = 0
    for b in range(len(I)):
        a = (logits[b], cost[b], table, int(I[b]), int(O[b]), mt, zid, allow_skip, test_mode)
        dp, bf = R.expected_cost(*a), R.brute_force(*a)
        assert dp["feasible"] == bf["feasible"]
        sc = R.scale(logits[b], cost[b], int(I[b]), zid, allow_skip)
        if not dp["feasible"]:
            for r in (dp, bf):
                assert r["risk"] == 0.0 and np.isposinf(r["loss"])
                assert not r["grad_logits"].any() and not r["grad_cost"].any()
            continue
        _close(dp, bf, sc, "dp vs brute force")
        feasible += 1
        _close(dp, R.torch_double_backward(*a), sc, "dp vs double backward")
        n = int(I[b])
        assert np.allclose(dp["grad_cost"][:n].sum(axis=1), 1.0, atol=TOL)
        assert np.allclose(dp["grad_logits"][:n].sum(axis=1), 0.0, atol=TOL * sc)
        assert not dp["grad_cost"][n:].any() and not dp["grad_logits"][n:].any()
        if not allow_skip:
            assert not dp["grad_cost"][:, zid].any() and not dp["grad_logits"][:, zid].any()
    assert feasible >= 1


@pytest.mark.parametrize("mode", sorted(MODES))
def test_entropy_is_minus_loss_minus_the_risk_of_the_logits(mode):
    tm, sk = MODES[mode]
    logits, _, table, I, O, mt, zid, allow_skip, test_mode = _tiny(1, tm, sk)
    h, gh = R.entropy_batch(logits, table, I, O, mt, zid, allow_skip, test_mode)
    for b in range(len(I)):
        bf = R.brute_force(logits[b], np.where(np.isfinite(logits[b]), logits[b], 0.0), table, int(I[b]),
                           int(O[b]), mt, zid, allow_skip, test_mode)
        if not bf["feasible"]:
            assert np.isneginf(h[b]) and not gh[b].any()
            continue
        assert abs(h[b] - bf["entropy"]) <= TOL * max(1.0, abs(bf["entropy"]))
        assert h[b] >= -TOL
        assert np.max(np.abs(gh[b] + bf["grad_logits"])) <= TOL * 50  # dH = -(d risk - posterior)


def test_infeasible_rows_follow_the_rule():
    c = C.infeasible()
    r = C.reference(c)
    assert list(r["feasible"]) == [True, False, True, False, True, False, False]
    for b in (1, 3, 5, 6):
        assert r["risk"][b] == 0.0 and np.isposinf(r["loss"][b])
        assert not r["grad_logits"][b].any() and not r["grad_cost"][b].any()
        bf = R.brute_force(c["logits"][b], c["cost"][b], c["table"], int(c["I"][b]), int(c["O"][b]), c["mt"],
                           c["zid"], c["allow_skip"], c["test_mode"])
        assert not bf["feasible"]
    # a length outside the tensor and a negative duration: no lattice either
    a = (c["logits"][0], c["cost"][0])
    assert not R.expected_cost(*a, c["table"], 7, 18, 18, 0, True, False)["feasible"]
    assert not R.expected_cost(*a, c["table"], 6, -1, 18, 0, True, False)["feasible"]
    assert not R.expected_cost(*a, np.array([0, 1, -2, 3]), 6, 12, 18, 0, True, False)["feasible"]


def test_dead_classes_never_reach_a_result():
    logits, cost, table, I, O, mt, zid, _, _ = _tiny(1, False, False)
    ref = R.expected_cost_batch(logits, cost, table, I, O, mt, zid, False, False)
    bad = cost.copy()
    bad[:, :, zid] = np.nan                      # the zero class under no-skip
    bad[np.isneginf(logits)] = np.inf            # classes of weight zero
    got = R.expected_cost_batch(logits, bad, table, I, O, mt, zid, False, False)
    for k in ("risk", "loss", "grad_logits", "grad_cost", "scale"):
        assert np.array_equal(got[k], ref[k]), k


def test_constant_and_zero_cost():
    logits, cost, table, I, O, mt, zid, _, _ = _tiny(2, True, True)
    z = R.expected_cost_batch(logits, np.zeros_like(cost), table, I, O, mt, zid, True, True)
    assert not z["risk"].any() and not z["grad_logits"].any() and z["grad_cost"].any()
    k = R.expected_cost_batch(logits, np.full_like(cost, 2.5), table, I, O, mt, zid, True, True)
    f = k["feasible"]
    assert np.allclose(k["risk"][f], 2.5 * I[f], atol=TOL * 20) and np.abs(k["grad_logits"]).max() <= TOL * 20


def test_the_shared_cases_are_what_the_issue_lists():
    names = set(C.case_makers(lambda D: 64 if D <= 32 else 32))
    assert {f"classes-{D}" for D in (1, 3, 8, 9, 16, 17, 33, 64)} <= names
    assert {f"chunk-4-{I}" for I in (1, 2, 63, 64, 65, 129)} <= names
    assert {f"chunk-40-{I}" for I in (1, 2, 31, 32, 33, 65)} <= names
    assert {"wide", "long-test0", "long-test1", "infeasible", "exponent", "cancellation", "constant"} <= names
    assert set(C.VALUE_NAMES) <= names and len(C.VALUE_NAMES) == 12
    for name in C.VALUE_NAMES:  # the float64 reference is feasible and finite on every value class
        c = C.case_makers(lambda D: 64)[name]()
        r = C.reference(c)
        assert r["feasible"].all(), name
        assert all(np.isfinite(r[k]).all() for k in ("risk", "loss", "grad_logits", "grad_cost", "scale")), name
        n = c["I"]
        for b in range(len(n)):
            assert np.allclose(r["grad_cost"][b, :n[b]].sum(axis=1), 1.0, atol=TOL), name
    w = C.wide()
    assert w["test_mode"] and w["logits"].shape[1:] == (48, 16) and w["mt"] + 1 > 512
