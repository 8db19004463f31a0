"""Inputs of the v2 expected-cost GPU tests (tests/test_gpu_v2_expected_cost.py), shared with
tools/bench_v2_expected_cost.py --accuracy, which measures on exactly these cases the errors the
tests' tolerances come from. Each case is the smallest shape at which its mechanism can go wrong.
Pure numpy; the float64 reference is tests/v2_expected_cost_ref.py. Test infrastructure only."""
import numpy as np

import f4_cases
import v2_expected_cost_ref as R
import value_cases as VC

CLASS_DS = (1, 3, 8, 9, 16, 17, 33, 64)   # every instantiation of the class count and its padding
CHUNK_DS = (4, 40)                        # 64-step and 32-step staging chunks
OUTPUTS = ("risk", "loss", "grad_logits", "grad_cost")
SMALL_TABLE = np.array([0, 1, 3, 5], np.int32)  # four classes whose totals can follow the band


def costs(B, T, D, seed):
    return np.random.default_rng(seed + 7).standard_normal((B, T, D)).astype(np.float32)


def make(logits, I, O, table, mt=None, allow_skip=True, test_mode=False, cost=None, zid=0, seed=0):
    B, T, D = logits.shape
    O = np.asarray(O, np.int32)
    return {"logits": np.asarray(logits, np.float32),
            "cost": costs(B, T, D, seed) if cost is None else np.asarray(cost, np.float32),
            "table": np.asarray(table, np.int32), "I": np.asarray(I, np.int32), "O": O,
            "mt": int(O.max()) if mt is None else int(mt), "zid": zid, "allow_skip": allow_skip,
            "test_mode": test_mode}


def lengths(rng, B, Imax, full=True):
    """ragged input lengths (the first one Imax) and band-mode output lengths that leave paths:
    O >= 3 (I - 1), or the overrun rule empties the lattice; totals near 3.2 .. 4.5 per step"""
    I = rng.integers(1, Imax + 1, size=B).astype(np.int32)
    if full:
        I[0] = Imax
    O = np.array([int(i * rng.uniform(3.2, 4.5)) for i in I], np.int32)
    return I, O


def classes(D):
    """ragged, I <= 9; D = 1: the one class (duration 3) at every step; durations 2, 3, 5 for
    D = 3, so that totals of 3 and more per step exist"""
    rng = np.random.default_rng(D)
    if D == 1:
        I = np.array([9, 4, 1], np.int32)
        return make(np.log(rng.uniform(0.2, 1.0, (3, 9, 1))), I, 3 * I, [3], seed=D)
    logits, _, _ = f4_cases.random_case(rng, 3, 9, D)
    I, O = lengths(rng, 3, 9)
    table = np.arange(D) if D >= 8 else np.array([2, 3, 5, 4, 1, 6, 0])[:D]
    return make(logits, I, O, table, allow_skip=(D % 2 == 1), seed=D)


def chunk_Is(ch):
    return sorted({1, 2, ch - 1, ch, ch + 1, 2 * ch + 1})


def chunk(D, I):
    """two utterances, I and I - 1 steps, band mode; durations 0..D-1 with totals near 3 I"""
    rng = np.random.default_rng(100 * D + I)
    logits, _, _ = f4_cases.random_case(rng, 2, I, D)
    Is = np.array([I, max(1, I - 1)], np.int32)
    O = np.array([3 * I + 2, 4 * max(1, I - 1)], np.int32)
    return make(logits, Is, O, np.arange(D) if D > 4 else SMALL_TABLE[:D], seed=100 * D + I)


def wide():
    """test mode, I = 48, durations 0..15: windows wider than the 512 threads of a sweep"""
    rng = np.random.default_rng(48)
    logits = np.log(rng.dirichlet(np.ones(16), size=(2, 48))).astype(np.float32)
    return make(logits, [48, 47], [300, 320], np.arange(16), mt=719, test_mode=True, seed=48)


def long_durations(test_mode):
    """durations above 64 (the clamped cell form), I = 6"""
    rng = np.random.default_rng(6)
    logits, _, _ = f4_cases.random_case(rng, 3, 6, 4)
    O = [420, 350, 200] if not test_mode else [300, 200, 131]
    return make(logits, [6, 5, 2], O, [0, 1, 70, 130], mt=(420 if not test_mode else 333),
                test_mode=test_mode, seed=6)


def mode(test_mode, allow_skip):
    rng = np.random.default_rng(5)
    logits, _, _ = f4_cases.random_case(rng, 4, 6, 4)
    I, O = lengths(rng, 4, 6)
    mt = int(O.max()) + (5 if test_mode else 0)   # test mode: max_total above max(O)
    return make(logits, I, O, [0, 1, 3, 5], mt=mt, allow_skip=allow_skip, test_mode=test_mode, seed=5)


def infeasible():
    """rows 0, 2, 4 feasible; 1: I = 0; 3: band O > max_total; 5: a step of -inf alone; 6: overrun"""
    rng = np.random.default_rng(9)
    logits, _, _ = f4_cases.random_case(rng, 7, 6, 4)
    logits[5, 2, :] = -np.inf
    I = np.array([6, 0, 5, 6, 3, 6, 6], np.int32)
    O = np.array([18, 7, 15, 25, 9, 17, 3], np.int32)
    return make(logits, I, O, [0, 1, 3, 5], mt=18, seed=9)


def exponent():
    """logits shifted by -80 per step at I = 64: alpha leaves the f32 exponent range"""
    rng = np.random.default_rng(64)
    logits, _, _ = f4_cases.random_case(rng, 2, 64, 8)
    logits = (logits - np.float32(80.0)).astype(np.float32)
    return make(logits, [64, 50], [200, 170], np.arange(8), seed=64)


def cancellation():
    """costs of +-1e3 with alternating sign at I = 32"""
    rng = np.random.default_rng(32)
    logits, _, _ = f4_cases.random_case(rng, 2, 32, 8)
    t, i = np.meshgrid(np.arange(32), np.arange(8), indexing="ij")
    cost = np.broadcast_to(np.where((t + i) % 2 == 0, 1e3, -1e3).astype(np.float32), (2, 32, 8)).copy()
    return make(logits, [32, 20], [100, 70], np.arange(8), cost=cost, seed=32)


def constant():
    """one cost on every move at I = 65: risk = k I, and grad_logits is the rounding noise of the
    means (each about k t) against the risk, the largest normalised grad_logits error there is"""
    c = chunk(4, 65)
    c["cost"] = np.full_like(c["cost"], np.float32(2.5))
    return c


def value(name, test_mode):
    """One input value class of tests/value_cases.py (its TOLERANCE_CLASSES) on the teacher-forced
    logits of v2_sample_ref.value_case: B=4, I=32 ragged, D=8, durations 0..7; costs N(0, 1)."""
    import v2_sample_ref
    logits, table, I, O, mt, allow_skip, tm = v2_sample_ref.value_case(name, test_mode)
    return make(logits, I, O, table, mt=mt, allow_skip=allow_skip, test_mode=tm, seed=32)


VALUE_NAMES = [f"value-{n}-test{tm}" for n in VC.TOLERANCE_CLASSES for tm in (0, 1)]

MODES = {"band": (False, True), "test_mode": (True, True), "band-noskip": (False, False),
         "test_mode-noskip": (True, False)}  # name -> (test_mode, allow_skip)


def tiny(seed, test_mode, allow_skip, D=4, Imax=6):
    """D <= 4, I <= 6, for the brute force over all D^I class sequences: logits, cost (float64),
    table, I, O, max_total, zero_duration_id, allow_skip, test_mode; odd seeds hold a dead class"""
    rng = np.random.default_rng(seed)
    logits, _, _ = f4_cases.random_case(rng, 4, Imax, D)
    I, O = lengths(rng, 4, Imax)
    if seed % 2:
        logits[:, 1, 1] = -np.inf
    cost = rng.standard_normal(logits.shape) * 3.0
    mt = int(O.max()) + (2 if test_mode else 0)
    return logits, cost, SMALL_TABLE[:D], I, O, mt, 0, allow_skip, test_mode


def case_makers(chunk_steps):
    """name -> function making the case, for every shape the GPU tests compare with the reference;
    chunk_steps(D) is the sweep's staging depth (ssnt_v2_expected_cost_chunk_steps of the A/B
    build)."""
    out = {f"classes-{D}": (lambda D=D: classes(D)) for D in CLASS_DS}
    for D in CHUNK_DS:
        for I in chunk_Is(chunk_steps(D)):
            out[f"chunk-{D}-{I}"] = lambda D=D, I=I: chunk(D, I)
    out["wide"] = wide
    for tm in (False, True):
        out[f"long-test{int(tm)}"] = lambda tm=tm: long_durations(tm)
        for sk in (False, True):
            out[f"mode-test{int(tm)}-skip{int(sk)}"] = lambda tm=tm, sk=sk: mode(tm, sk)
    out["infeasible"] = infeasible
    out["exponent"] = exponent
    out["cancellation"] = cancellation
    out["constant"] = constant
    for n in VC.TOLERANCE_CLASSES:
        for tm in (0, 1):
            out[f"value-{n}-test{tm}"] = lambda n=n, tm=tm: value(n, bool(tm))
    return out


def all_cases(chunk_steps):
    return {name: f() for name, f in case_makers(chunk_steps).items()}


def reference(c):
    return R.expected_cost_batch(c["logits"], c["cost"], c["table"], c["I"], c["O"], c["mt"], c["zid"],
                                 c["allow_skip"], c["test_mode"])


def errors(got, ref):
    """Worst normalised error per output over the batch, as expected_cost_cases.errors:
    |risk - ref| / scale_b; the largest |grad_logits - ref| of the utterance / scale_b; plain for
    grad_cost (a probability); for loss |loss - ref| / max(|ref|, 1): relative above 1, absolute
    below (an infeasible utterance must be +inf on both sides). The emit/shift measure is relative
    down to a reference of exactly 0; here test mode with skips admits every class sequence, so
    Z = 1 and the reference loss is a rounding residue near 1e-8, against which the one ulp(1) of
    absolute error that ln Z carries would read as a relative error of order 1."""
    sc = ref["scale"]
    e = {}
    e["risk"] = float(np.max(np.abs(got["risk"].astype(np.float64) - ref["risk"]) / sc))
    gl, rl = got["loss"].astype(np.float64), ref["loss"]
    fin = np.isfinite(rl)
    assert np.array_equal(np.isposinf(gl), ~fin), (gl, rl)
    den = np.maximum(np.abs(rl[fin]), 1.0)
    e["loss"] = float(np.max(np.abs(gl[fin] - rl[fin]) / den, initial=0.0))
    for k in ("grad_logits", "grad_cost"):
        if k in got and k in ref:
            d = np.abs(got[k].astype(np.float64) - ref[k]).reshape(len(sc), -1).max(axis=1)
            e[k] = float(np.max(d / (1.0 if k == "grad_cost" else sc)))
    return e
