"""The CPU references on the input value classes of tests/value_cases.py: every condition the GPU
tests of tests/test_gpu_value_ranges.py (and the value cases of the sampler and expected-cost
files) rely on holds for the references alone, so a GPU failure there cannot be the reference's.

  split-exponent oracle vs the float64 DP   the comparisons and bars of test_oracle_fwd_bwd.py
  v2 oracle vs v2_fwd_bwd_f64               the bars of test_oracle_v2_fwd_bwd.py::test_xf_vs_f64_medium
  NaN, < -1e6, > +1e6                       the oracles read them as -inf / +1e6, bit for bit
  the sampler's value cases                 unclear share within sample_cases.CAP_CASE
No GPU."""
import functools

import numpy as np
import pytest

import sample_cases as SC
import value_cases as VC
from test_oracle_fwd_bwd import _xf_vs_f64

F_TERM = 1
B, T, U = 3, 60, 24
S0, P0 = [60, 50, 24], [24, 20, 24]


@functools.lru_cache(maxsize=None)
def _base(shape, seed=0):
    import oracle as O
    return O.synth_log_trans(*shape, seed=seed)


def _usual_obs(shape, seed=3):
    return (np.random.default_rng(seed).standard_normal(shape) * 15 - 40).astype(np.float32)


def _same_bits(a, b):
    assert set(a) == set(b)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def _check(oracle, lt, S, P, lo, flags, cleaned):
    """xf vs float64 with the bars of test_oracle_fwd_bwd.py; for the classes that hold NaN or
    values outside [-1e6, +1e6] float64 gets what xf_exp reads them as, and the oracle must return
    the same bits on either form."""
    if cleaned:
        ltc, loc = VC.cleaned(lt), VC.cleaned(lo)
        _same_bits(oracle.fwd_bwd_xf(lt, S, P, log_obs=lo, flags=flags, debug=True),
                   oracle.fwd_bwd_xf(ltc, S, P, log_obs=loc, flags=flags, debug=True))
        lt, lo = ltc, loc
    return _xf_vs_f64(oracle, lt, S, P, lo=lo, flags=flags)


@pytest.mark.parametrize("flags", [F_TERM, 0])
@pytest.mark.parametrize("obs", [False, True])
@pytest.mark.parametrize("name", VC.LATTICE_CLASSES)
def test_lattice_classes_xf_vs_f64(oracle, name, obs, flags):
    lt = VC.lattice(name, _base((B, T, U)))
    lo = _usual_obs((B, T, U)) if obs else None
    a, _ = _check(oracle, lt, S0, P0, lo, flags, name in VC.CLEANED)
    if name not in VC.CLEANED:
        assert np.all(np.isfinite(a["loss"]))
    for kind in VC.length_kinds(name):  # the lengths the GPU tests run the class with
        S, P = VC.lengths(B, T, U, kind)
        _check(oracle, lt, S, P, lo, flags, name in VC.CLEANED)


def test_near_envelope_xf_vs_f64(oracle):
    ne = VC.NEAR_ENVELOPE
    lt = VC.lattice("near_envelope", _base(ne["shape"]))
    for flags in (F_TERM, 0):
        a, _ = _xf_vs_f64(oracle, lt, ne["S"], ne["P"], flags=flags)
        # the cumulative log-probability is past -2.9e8: an exponent below -4.2e8, above XF_EZERO
        assert np.all(a["loss"] > 2.9e8) and np.all(a["loss"] < 2.0 ** 29 * np.log(2.0))


@pytest.mark.parametrize("flags", [F_TERM, 0])
@pytest.mark.parametrize("trans", ["base", "peaked30"])
@pytest.mark.parametrize("name", list(VC.OBS))
def test_obs_classes_xf_vs_f64(oracle, name, trans, flags):
    lt = _base((B, T, U))
    if trans != "base":
        lt = VC.lattice(trans, lt)
    lo = VC.obs(name, (B, T, U))
    _check(oracle, lt, S0, P0, lo, flags, name in VC.CLEANED)
    S, P = VC.lengths(B, T, U)
    _check(oracle, lt, S, P, lo, flags, name in VC.CLEANED)


def _v2_medium(oracle, seed, test_mode, B=6, Imax=40, D=8):
    """The case of test_oracle_v2_fwd_bwd.py::test_xf_vs_f64_medium."""
    table = np.arange(D, dtype=np.int32)
    d = oracle.synth_durations(B, Imax, 4 * Imax, D, seed=seed)
    logits = oracle.synth_v2_step_logits(d, D, seed=seed)
    I = np.full(B, Imax, np.int32)
    I[1] = Imax - 7
    Ol = d.sum(1).astype(np.int32)
    Ol[1] = int(d[1, :I[1]].sum())
    return logits, table, I, Ol, int(Ol.max()) + (20 if test_mode else 0)


@pytest.mark.parametrize("test_mode", [False, True])
@pytest.mark.parametrize("name", list(VC.V2) + list(VC.V2_EXTRA))
def test_v2_classes_xf_vs_f64(oracle, name, test_mode):
    base, table, I, Ol, mt = _v2_medium(oracle, 0, test_mode)
    logits = VC.v2(name, base)
    xf = oracle.v2_fwd_bwd(logits, table, I, Ol, mt, 0, True, test_mode, debug=True)
    if name in VC.CLEANED:
        clean = VC.cleaned(logits)
        _same_bits(xf, oracle.v2_fwd_bwd(clean, table, I, Ol, mt, 0, True, test_mode, debug=True))
        logits = clean
    f64 = oracle.v2_fwd_bwd_f64(logits, table, I, Ol, mt, 0, True, test_mode)
    fin = np.isfinite(f64["loss"])
    assert np.array_equal(np.isfinite(xf["loss"]), fin) and np.all(np.isposinf(xf["loss"][~fin]))
    assert fin.all() or name in VC.CLEANED
    np.testing.assert_allclose(xf["loss"][fin], f64["loss"][fin], rtol=2e-6, atol=1e-5)
    np.testing.assert_allclose(xf["grad"], f64["grad"], atol=1e-5)
    for b in np.flatnonzero(fin):  # posterior mass 1 per step
        mass = -xf["grad"][b, :I[b]].sum(-1)
        assert np.max(np.abs(mass - 1.0)) < 1e-4
        assert not xf["grad"][b, I[b]:].any()


@pytest.mark.parametrize("name", VC.TOLERANCE_CLASSES)
def test_sampler_value_cases_are_clear(name):
    # a condition of the GPU test, not a measurement: B=4, T=48, U=20, K=16, uniforms seed 7
    c = SC.value(name)
    n, t = SC.unclear_share(c)
    print(f"{name}: {n} of {t} unclear")
    assert c["ref"]["feasible"].all() and t == 4 * 16
    assert n <= SC.CAP_CASE * t


def test_as_neg_inf_and_as_clamped_change_exactly_their_cells():
    nxt = np.nextafter(np.float32(-1e6), np.float32(-np.inf))
    up = np.nextafter(np.float32(1e6), np.float32(np.inf))
    x = np.array([0.0, -0.0, -1e6, nxt, -np.inf, np.nan, 1e6, up, 1e30, np.inf, -3e38, 88.0, -103.0],
                 np.float32)
    x = np.concatenate([x, np.array([0xFFFFFFFF, 0x7F800001], np.uint32).view(np.float32)])  # NaN payloads
    n = VC.as_neg_inf(x)
    dead = np.isnan(x) | (x < np.float32(-1e6))
    assert dead.tolist() == [False, False, False, True, True, True, False, False, False, False, True,
                             False, False, True, True]
    assert np.all(np.isneginf(n[dead])) and n[~dead].tobytes() == x[~dead].tobytes()
    c = VC.as_clamped(x)
    high = x > np.float32(1e6)
    assert np.flatnonzero(high).tolist() == [7, 8, 9]
    assert np.all(c[high] == np.float32(1e6)) and c[~high].tobytes() == x[~high].tobytes()
    assert n.dtype == c.dtype == np.float32 and n is not x and c is not x
    # on the classes themselves: only `threshold` and the NaN classes hold such cells
    base = _base((B, T, U))
    for name in VC.LATTICE_CLASSES:
        lt = VC.lattice(name, base)
        changed = VC.cleaned(lt).tobytes() != lt.tobytes()
        assert changed == (name in VC.CLEANED), name
    t = VC.lattice("threshold", base)
    share = np.mean(t.view(np.uint32) != base.view(np.uint32))
    assert 0.08 < share < 0.12
    for v in VC.THRESHOLD_VALUES:  # each of the six values is there, in equal numbers (+-1)
        assert abs(int(np.sum(t.view(np.uint32) == v.view(np.uint32))) - share * t.size / 6) <= 1


def test_lengths_cover_the_normalisation_period():
    for shape in [(4, 48, 64), (4, 48, 80), (4, 48, 160), (3, 40, 256), (3, 320, 80), (2, 40, 300), (2, 30, 700)]:
        Bn, Tn, Un = shape
        for kind in ("ragged", "diag", "single"):
            S, P = VC.lengths(*shape, kind)
            assert len(set(int(s) % 4 for s in S)) == min(Bn, 4), (shape, kind)
            assert np.all(P >= 1) and np.all(P <= S) and np.all(S <= Tn) and np.all(P <= Un), (shape, kind)
        S, P = VC.lengths(*shape)
        assert S[0] == Tn and P[0] == min(Un, Tn - Tn // 4) and S[-1] == P[-1]
        assert Bn < 4 or P[2] == 1
        S, P = VC.lengths(*shape, "diag")
        assert np.array_equal(S, P)
