"""Inputs of the expected-cost GPU tests (tests/test_gpu_expected_cost.py), shared with
tools/bench_expected_cost.py --accuracy, which measures on exactly these cases the errors the
tests' tolerances come from. Each case is the smallest shape at which its mechanism can go wrong.
Pure numpy; the float64 reference is tests/expected_cost_ref.py. Test infrastructure only."""
import numpy as np

import expected_cost_ref as R
import value_cases as VC

LANE_US = (1, 2, 63, 64, 65, 128, 129, 257, 513, 1024)
CHUNK_US = (5, 130)
OUTPUTS = ("risk", "loss", "grad_trans", "grad_cost", "grad_obs")
VALUE_NAMES = [f"value-{n}" for n in VC.TOLERANCE_CLASSES]


def lattice(B, T, U, seed, obs=False):
    rng = np.random.default_rng(seed)
    lt = np.log(rng.dirichlet([1.5, 1.0], size=(B, T, U))).astype(np.float32)
    lo = (0.5 * rng.standard_normal((B, T, U))).astype(np.float32) if obs else None
    return lt, lo


def costs(B, T, U, seed):
    return np.random.default_rng(seed + 7).standard_normal((B, T, U, 2)).astype(np.float32)


def ragged(B, T, U, seed):
    """The full lattice, S = P, then random extents."""
    rng = np.random.default_rng(seed + 13)
    m = min(T, U)
    P = [m, m] + [int(x) for x in rng.integers(1, m + 1, size=max(B - 2, 0))]
    S = [T, m] + [int(rng.integers(p, T + 1)) for p in P[2:]]
    return np.array(S[:B], np.int32), np.array(P[:B], np.int32)


def make(B, T, U, seed, obs, terminal=True, S=None, P=None):
    lt, lo = lattice(B, T, U, seed, obs)
    if S is None:
        S, P = ragged(B, T, U, seed)
    return {"lt": lt, "lo": lo, "cost": costs(B, T, U, seed), "S": np.asarray(S, np.int32),
            "P": np.asarray(P, np.int32), "terminal": terminal}


def lane(U):
    return make(3, U + 3, U, U, obs=(U % 2 == 1))


def chunk_Ts(R):
    return sorted({1, 2, 3, R, R + 1, 2 * R + 1})


def chunk(U, T):
    return make(2, T, U, 100 * U + T, obs=(T % 2 == 0), S=[T, max(1, T - 1)],
                P=[min(U, T), max(1, min(U, T - 1) - 1)])


def mode(obs, terminal):
    return make(4, 7, 4, 5, obs, terminal, S=[7, 4, 6, 1], P=[4, 4, 2, 1])


def exponent():
    """log_trans about -80 per step at T = 64: alpha leaves the f32 exponent range."""
    c = make(2, 64, 8, 64, obs=True, S=[64, 50], P=[8, 5])
    c["lt"] = (c["lt"] - np.float32(80.0)).astype(np.float32)
    return c


def cancellation():
    """costs of +-1e3 with alternating sign at T = 32, U = 8."""
    c = make(2, 32, 8, 32, obs=False, S=[32, 20], P=[8, 8])
    s, p, k = np.meshgrid(np.arange(32), np.arange(8), np.arange(2), indexing="ij")
    c["cost"] = np.broadcast_to(np.where((s + p + k) % 2 == 0, 1e3, -1e3).astype(np.float32), (2, 32, 8, 2)).copy()
    return c


def value(name):
    """One input value class of tests/value_cases.py (its TOLERANCE_CLASSES) at B=4, T=48, U=20:
    ragged lengths, S mod 4 = 0, 3, 2, 1; the costs are the usual N(0, 1)."""
    B, T, U = 4, 48, 20
    S, _ = VC.lengths(B, T, U)
    c = make(B, T, U, 48, obs=False, S=S, P=[20, 13, 7, 12])
    c["lt"] = VC.lattice(name, c["lt"])
    return c


def case_makers(chunk_rows):
    """name -> function making the case, for every shape the GPU tests compare with the reference;
    chunk_rows(U, obs) is the sweep's chunk depth (ssnt_expected_cost_chunk_rows of the A/B
    build)."""
    out = {f"lane-{U}": (lambda U=U: lane(U)) for U in LANE_US}
    for U in CHUNK_US:
        Ts = set()
        for obs in (False, True):
            Ts |= set(chunk_Ts(chunk_rows(U, obs)))
        for T in sorted(Ts):
            out[f"chunk-{U}-{T}"] = lambda U=U, T=T: chunk(U, T)
    for obs in (False, True):
        for terminal in (False, True):
            out[f"mode-obs{int(obs)}-term{int(terminal)}"] = lambda obs=obs, terminal=terminal: mode(obs, terminal)
    out["exponent"] = exponent
    out["cancellation"] = cancellation
    for name in VC.TOLERANCE_CLASSES:
        out[f"value-{name}"] = lambda name=name: value(name)
    return out


def all_cases(chunk_rows):
    return {name: f() for name, f in case_makers(chunk_rows).items()}


def reference(c):
    return R.expected_cost_batch(c["lt"], c["cost"], c["S"], c["P"], c["lo"], c["terminal"])


def errors(got, ref):
    """Worst normalised error per output over the batch: |risk - ref| / scale_b; the largest
    |grad - ref| of the utterance / scale_b for grad_trans and grad_obs; plain for grad_cost (a
    probability); relative for loss (absolute where the reference is exactly 0; an infeasible
    utterance must be +inf on both sides)."""
    sc = ref["scale"]
    e = {}
    e["risk"] = float(np.max(np.abs(got["risk"].astype(np.float64) - ref["risk"]) / sc))
    gl, rl = got["loss"].astype(np.float64), ref["loss"]
    fin = np.isfinite(rl)
    assert np.array_equal(np.isposinf(gl), ~fin), (gl, rl)
    den = np.where(rl[fin] == 0, 1.0, np.abs(rl[fin]))
    e["loss"] = float(np.max(np.abs(gl[fin] - rl[fin]) / den, initial=0.0))
    for k in ("grad_trans", "grad_cost", "grad_obs"):
        if k in got and k in ref:
            d = np.abs(got[k].astype(np.float64) - ref[k]).reshape(len(sc), -1).max(axis=1)
            e[k] = float(np.max(d / (1.0 if k == "grad_cost" else sc)))
    return e
