"""CPU checks for the v2 posterior sampler: the new symbols exist everywhere they
must, the workspace query is F4's forward rows plus Z, the float64 reference of
tests/v2_sample_ref.py draws every admissible sequence of the tiny cases with its posterior
probability, and the redrawn uniforms of `clear_uniforms` leave (almost) every sample of every
family the GPU file uses clear. No GPU."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import v2_sample_ref as SR
import v2_viterbi_ref as VR

ROOT = Path(__file__).resolve().parent.parent
NEW = ["ssnt_v2_sample_align_workspace_size", "ssnt_v2_sample_align_device"]


def test_new_symbols_everywhere():
    import ssnt_tts_amd
    from ssnt_tts_amd._lib import SIGNATURES, load
    header = (ROOT / "include" / "ssnt_tts_c.h").read_text()
    lib = ROOT / "ssnt-tts-rust_amd" / "lib" / "libssnt_tts_c.so"
    out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
    for s in NEW:
        assert re.search(rf"\b{s}\s*\(", header), s
        assert re.search(rf"\bT {s}$", out, flags=re.M), s
        assert s in SIGNATURES and getattr(load(), s) is not None, s
    assert "v2_sample_align" in ssnt_tts_amd.__all__ and callable(ssnt_tts_amd.v2_sample_align)
    assert "New: the reference has no sampler." in header


def _wcap(max_total, test_mode):  # v2_lattice_dev.h v2_fwd_bwd_wcap
    X = max_total + 1
    return X if test_mode else min(int(0.15 * max_total) + 8, X)


def test_workspace_query_host_only():
    from ssnt_tts_amd._lib import load
    q = load().ssnt_v2_sample_align_workspace_size
    for B in (0, -1):
        assert q(B, 400, 2000, False, 16) == 0
    # F4's forward rows + Z: alpha (B, I+1, Wcap) and Z (B), 8 bytes each
    for B, I, mt, tm, K in [(64, 400, 2000, False, 16), (3, 150, 777, True, 1)]:
        assert q(B, I, mt, tm, K) == (B * (I + 1) * _wcap(mt, tm) + B) * 8
        f4 = load().ssnt_v2_fwd_bwd_workspace_size(B, I, mt, tm)
        assert f4 == (2 * B * (I + 1) * _wcap(mt, tm) + B) * 8  # (F4 keeps the beta rows too)
    base = (4, 50, 300, False, 4)
    for pos, bigger in [(0, 5), (1, 51), (2, 301), (3, True), (4, 5), (4, 64)]:
        more = list(base)
        more[pos] = bigger
        assert q(*more) >= q(*base) > 0, (pos, bigger)
    assert q(4, 50, 300, False, 1) == q(4, 50, 300, False, 64)  # not a function of the sample count


@pytest.mark.parametrize("mode", VR.MODES)
def test_reference_frequencies_match_the_posterior(mode):
    N = 8192
    checked = 0
    for seed in range(6):
        case = VR.tiny_case(seed, mode)
        logits, table, I, O, mt, allow_skip, test_mode = case
        B, T, _ = logits.shape
        u = np.random.default_rng([77, seed]).random((B, N, T + 1), dtype=np.float32)
        r = SR.sample_batch(case, u)
        for b in range(B):
            post = SR.path_posterior(logits[b], table, int(I[b]), int(O[b]), mt, 0, allow_skip, test_mode)
            assert bool(post) == bool(r["feasible"][b]), (seed, b)
            if not post:
                assert np.all(r["total"][b] == -1) and np.all(r["duration_class"][b] == -1)
                continue
            dev = SR.frequency_deviation(r["duration_class"][b], r["total"][b], int(I[b]), post)
            assert dev <= 5.0, (seed, b, dev)
            checked += 1
    assert checked >= 36, checked  # half of the mode's 72 utterances


def test_reference_paths_are_admissible_and_summed_in_f32():
    case = VR.tiny_case(3, "band")
    logits, table, I, O, mt, allow_skip, test_mode = case
    u = np.random.default_rng(5).random((len(I), 4, logits.shape[1] + 1), dtype=np.float32)
    r = SR.sample_batch(case, u)
    assert r["feasible"].any()
    for b in np.flatnonzero(r["feasible"]):
        n = int(I[b])
        for k in range(4):
            cls = r["duration_class"][b, k]
            assert np.all(cls[:n] >= 0) and np.all(cls[n:] == -1)
            assert int(r["duration"][b, k].sum()) == int(r["total"][b, k]) == int(O[b])
            lp = SR.path_log_prob_f32(logits[b], cls)
            s64 = sum(float(logits[b, t, cls[t]]) for t in range(n))
            assert lp.dtype == np.float32 and abs(float(lp) - s64) <= 1e-5 * max(1.0, abs(s64))


def test_clamp():
    u = np.array([1.0, np.nan, -1.0, 0.25, 2.0], np.float32)
    assert np.array_equal(SR.clamp_uniform(u), np.array([SR.U_MAX, 0, 0, 0.25, SR.U_MAX], np.float32))


@pytest.mark.parametrize("name", sorted(SR.FAMILIES))
def test_redrawn_uniforms_leave_the_family_clear(name):
    case, K, u, res = SR.family(name)
    feasible = res["feasible"]
    clear = SR.clear(res)
    want = int(feasible.sum()) * K
    assert clear.sum() >= 0.99 * want, (name, int(clear.sum()), want)
    assert u.dtype == np.float32 and u.shape == (len(feasible), K, case[0].shape[1] + 1)
    u2, res2 = SR.clear_uniforms(case, K, 0)  # deterministic
    assert np.array_equal(u, u2) and np.array_equal(res["duration_class"], res2["duration_class"])


def test_value_families_are_the_tolerance_classes():
    import value_cases as VC
    assert SR.VALUE_CLASSES == VC.TOLERANCE_CLASSES
    for n in VC.TOLERANCE_CLASSES:
        for mode in ("band", "test_mode"):
            case, K, _, res = SR.family(f"value-{n}-{mode}")
            assert K == 16 and case[0].shape == (4, 32, 8) and res["feasible"].all(), (n, mode)


def _family_of(name):  # the tiny cases are one family per mode, over their six seeds
    return re.sub(r"^tiny-\d+-", "tiny-", name)


@pytest.mark.parametrize("fam", sorted({_family_of(n) for n in SR.FAMILIES}))
def test_half_of_every_family_is_feasible(fam):
    feasible = np.concatenate([SR.family(n)[3]["feasible"] for n in sorted(SR.FAMILIES) if _family_of(n) == fam])
    assert 2 * int(feasible.sum()) >= len(feasible), (fam, feasible)
