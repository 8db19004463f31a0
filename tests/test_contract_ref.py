"""The CPU references never read a dead cell: each returns bit-identical outputs on a clean input
and on the same input with every cell class of tests/contract_cases.py overwritten by NaN (two
patterns), +inf, 1e30 and 88. The GPU contract tests (tests/test_gpu_contract.py) ask the same of
the kernels and compare them with references computed from the clean input only, which this file
justifies."""
import functools

import numpy as np
import pytest

import contract_cases as CC
import sample_cases as SC
import v2_viterbi_ref as V2R
import viterbi_ref as VR
from f4_cases import random_case

VALUE_IDS = list(CC.VALUES) + ["alternating"]


def _value(name, B):
    return CC.alternating(B) if name == "alternating" else CC.VALUES[name]


@functools.lru_cache(maxsize=None)
def _grid(name):
    """(lt, lo, S, P): the tiny exhaustive (S, P) grid at T = 7, U = 4, or B = 5, T = 30, U = 17
    ragged."""
    if name == "tiny":
        T, U = 7, 4
        SP = [(s, p) for s in range(T + 1) for p in range(U + 1)]
        S, P = [s for s, _ in SP], [p for _, p in SP]
    else:
        T, U = 30, 17
        S, P = [30, 22, 17, 9, 1], [17, 9, 17, 4, 1]
    lt, lo = SC.lattice(len(S), T, U, 3 + T, obs=True)
    return lt, lo, np.array(S), np.array(P)


GRIDS = ["tiny", "ragged"]


def test_the_helpers_dirty_what_they_say_and_nothing_else():
    lt, lo, S, P = _grid("ragged")
    for terminal in (True, False):
        d, do = CC.dirty_lattice(lt, lo, S, P, CC.VALUES["nan_ones"], terminal)
        mt, mo = CC.lattice_dead_mask(lt.shape, S, P, terminal)
        assert np.all(d.view(np.uint32)[mt] == 0xFFFFFFFF) and np.array_equal(d[~mt], lt[~mt])
        assert np.all(do.view(np.uint32)[mo] == 0xFFFFFFFF) and np.array_equal(do[~mo], lo[~mo])
        for b in range(len(S)):
            s, p = int(S[b]), int(P[b])
            live = ~mt[b]
            assert live[:s - 1, :p - 1].all() and live[:s - 1, p - 1, 0].all()
            assert live[s - 1, p - 1, 0] == terminal
            assert live.sum() == (s - 1) * (2 * p - 1) + terminal
            assert (~mo[b]).sum() == s * p and not mo[b, :s, :p].any()
    d, _ = CC.dirty_lattice(lt, None, S, P, CC.alternating(5), True)
    mt, _ = CC.lattice_dead_mask(lt.shape, S, P, True)
    for b, want in enumerate([np.inf, 1e30, 88.0, np.inf, 1e30]):
        assert np.all(d[b][mt[b]] == np.float32(want))
    lg = np.zeros((3, 6, 4), np.float32)
    m = CC.v2_dead_mask(lg.shape, [6, 2, 0], 1, False)
    assert m.sum() == 4 * (0 + 4 + 6) + (6 + 2 + 0) and m[:, :, 1].all() and not m[0, :, [0, 2, 3]].any()
    assert CC.v2_dead_mask(lg.shape, [6, 2, 0], 1, True).sum() == 4 * (0 + 4 + 6)
    g = CC.dirty_v2(lg, [6, 2, 0], CC.VALUES["nan"], 1, False)
    assert np.all(g.view(np.uint32)[m] == 0x7FC00000) and not g[~m].any()
    assert not CC.same_bits(np.float32([0.0]), np.float32([-0.0]))
    assert CC.same_bits({"a": CC.VALUES["nan"]}, {"a": CC.VALUES["nan"]})
    assert not CC.same_bits(CC.VALUES["nan"], CC.VALUES["nan_ones"])


# ---- the emit/shift lattice -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _xf(oracle, grid, flags, obs):
    lt, lo, S, P = _grid(grid)
    return oracle.fwd_bwd_xf(lt, S, P, log_obs=lo if obs else None, flags=flags, debug=True)


@pytest.mark.parametrize("value", VALUE_IDS)
@pytest.mark.parametrize("obs", [False, True])
@pytest.mark.parametrize("flags", [1, 0, 3])
@pytest.mark.parametrize("grid", GRIDS)
def test_fwd_bwd_xf(oracle, grid, flags, obs, value):
    lt, lo, S, P = _grid(grid)
    d, do = CC.dirty_lattice(lt, lo if obs else None, S, P, _value(value, len(S)), bool(flags & 1))
    got = oracle.fwd_bwd_xf(d, S, P, log_obs=do, flags=flags, debug=True)
    assert CC.same_bits(got, _xf(oracle, grid, flags, obs))


@functools.lru_cache(maxsize=None)
def _f64(oracle, grid, flags, obs):
    lt, lo, S, P = _grid(grid)
    return oracle.fwd_bwd_f64(lt, S, P, log_obs=lo if obs else None, flags=flags)


@pytest.mark.parametrize("value", VALUE_IDS)
@pytest.mark.parametrize("obs", [False, True])
@pytest.mark.parametrize("flags", [1, 0, 3])
@pytest.mark.parametrize("grid", GRIDS)
def test_fwd_bwd_f64(oracle, grid, flags, obs, value):
    lt, lo, S, P = _grid(grid)
    d, do = CC.dirty_lattice(lt, lo if obs else None, S, P, _value(value, len(S)), bool(flags & 1))
    got = oracle.fwd_bwd_f64(d, S, P, log_obs=do, flags=flags)
    assert CC.same_bits(got, _f64(oracle, grid, flags, obs))


@pytest.mark.parametrize("value", VALUE_IDS)
@pytest.mark.parametrize("obs", [False, True])
@pytest.mark.parametrize("flags", [1, 0])
@pytest.mark.parametrize("grid", GRIDS)
def test_fwd_bwd_xf_state(oracle, grid, flags, obs, value):
    # what the debug64 entry is compared with
    lt, lo, S, P = _grid(grid)
    d, do = CC.dirty_lattice(lt, lo if obs else None, S, P, _value(value, len(S)), bool(flags & 1))
    got = oracle.fwd_bwd_xf_state(d, S, P, log_obs=do, flags=flags)
    assert CC.same_bits(got, oracle.fwd_bwd_xf_state(lt, S, P, log_obs=lo if obs else None, flags=flags))


@pytest.mark.parametrize("value", VALUE_IDS)
@pytest.mark.parametrize("obs", [False, True])
@pytest.mark.parametrize("terminal", [True, False])
@pytest.mark.parametrize("grid", GRIDS)
def test_viterbi_dp(grid, terminal, obs, value):
    lt, lo, S, P = _grid(grid)
    lo = lo if obs else None
    d, do = CC.dirty_lattice(lt, lo, S, P, _value(value, len(S)), terminal)
    assert CC.same_bits(VR.dp(d, S, P, do, terminal), VR.dp(lt, S, P, lo, terminal))


@pytest.mark.parametrize("value", VALUE_IDS)
@pytest.mark.parametrize("obs", [False, True])
@pytest.mark.parametrize("terminal", [True, False])
@pytest.mark.parametrize("grid", GRIDS)
def test_sampler_reference(grid, terminal, obs, value):
    lt, lo, S, P = _grid(grid)
    lo = lo if obs else None
    d, do = CC.dirty_lattice(lt, lo, S, P, _value(value, len(S)), terminal)
    a, b = SC._case(lt, lo, S, P, 4, 7, terminal)["ref"], SC._case(d, do, S, P, 4, 7, terminal)["ref"]
    for k in ("feasible", "position", "duration", "clear", "margin"):
        assert CC.same_bits(a[k], b[k]), k


# ---- the v2 duration-class lattice ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _v2(name, mode):
    """logits, table, I, O, max_total, allow_skip, test_mode: the tiny brute-force batch of
    v2_viterbi_ref, or B = 5, Imax = 30, D = 6 ragged."""
    if name == "tiny":
        return V2R.tiny_case(0, mode)
    logits, I, O = random_case(np.random.default_rng(30), 5, 30, 6)
    I[0], I[4] = 30, 1
    O[0], O[4] = 60, 2
    test_mode, allow_skip = mode == "test_mode", mode != "no_skip"
    return logits, np.arange(6, dtype=np.int32), I, O, int(O.max()) + (5 if test_mode else 0), allow_skip, test_mode


@pytest.mark.parametrize("value", VALUE_IDS)
@pytest.mark.parametrize("mode", V2R.MODES)
@pytest.mark.parametrize("grid", GRIDS)
def test_v2_fwd_bwd(oracle, grid, mode, value):
    logits, table, I, O, mt, allow_skip, test_mode = _v2(grid, mode)
    d = CC.dirty_v2(logits, I, _value(value, len(I)), 0, allow_skip)
    assert not CC.same_bits(d, logits)
    for flags in (0, 2):
        want = oracle.v2_fwd_bwd(logits, table, I, O, mt, 0, allow_skip, test_mode, flags=flags, debug=True)
        got = oracle.v2_fwd_bwd(d, table, I, O, mt, 0, allow_skip, test_mode, flags=flags, debug=True)
        assert CC.same_bits(got, want)


@pytest.mark.parametrize("value", VALUE_IDS)
@pytest.mark.parametrize("mode", V2R.MODES)
@pytest.mark.parametrize("grid", GRIDS)
def test_v2_viterbi_dp(grid, mode, value):
    logits, table, I, O, mt, allow_skip, test_mode = _v2(grid, mode)
    d = CC.dirty_v2(logits, I, _value(value, len(I)), 0, allow_skip)
    want = V2R.dp(logits, table, I, O, mt, 0, allow_skip, test_mode)
    assert CC.same_bits(V2R.dp(d, table, I, O, mt, 0, allow_skip, test_mode), want)
    assert grid == "tiny" or np.isfinite(want["log_prob"]).any()
