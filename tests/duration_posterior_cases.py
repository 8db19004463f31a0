"""Inputs of the duration-posterior GPU tests (tests/test_gpu_duration_posterior.py), shared with
tools/bench_duration_posterior.py --accuracy, which measures on exactly these cases the errors the
tests' tolerance comes from. Each case is the smallest shape at which its mechanism can go wrong.
Pure numpy; the float64 reference is tests/duration_posterior_ref.py. Test infrastructure only."""
import numpy as np

import duration_posterior_ref as R
import expected_cost_cases as EC
import value_cases as VC

LANE_US = (1, 2, 63, 64, 65, 129, 257, 1024)
# the kernel's forms change at D-1 = 16, 32, 64 (lanes per position) and 64, 128 (bins per lane)
BIN_DS_SHORT = (2, 3, 17, 18, 30)       # at T = 24: the tail alone, D = 3, a form edge, D > T
BIN_DS_LONG = (33, 34, 63, 64, 65, 66, 129, 130, 256)  # at T = 140: durations reach every form's lanes
OUTPUTS = ("dur_post", "loss")


def _case(c, D):
    return {"lt": c["lt"], "lo": c["lo"], "S": c["S"], "P": c["P"], "terminal": c["terminal"], "D": int(D)}


def make(B, T, U, D, seed, obs, terminal=True, S=None, P=None):
    return _case(EC.make(B, T, U, seed, obs, terminal, S, P), D)


def lane(U):
    """T = U + 3, ragged extents: no position holds more than 4 steps, D-1 = 3 cuts a true tail."""
    return make(3, U + 3, U, 4, U, obs=(U % 2 == 1))


def chunk_Ss(rows):
    return sorted({1, 2, 3, rows, rows + 1, 2 * rows + 1})


def chunk(S, tile):
    """P at the tile edge and one either side of it (P = tile: the first tile sweeps exactly S
    steps), and one position alone; T = S."""
    P = [max(1, min(S, p)) for p in (tile - 1, tile, tile + 1, 1)]
    return make(4, S, tile + 2, 8, 1000 + S, obs=(S % 2 == 0), S=[S] * 4, P=P)


def bins(D):
    if D in BIN_DS_SHORT:
        return make(2, 24, 6, D, 24, obs=(D % 2 == 0), S=[24, 20], P=[6, 3])
    return make(2, 140, 5, D, 140, obs=(D % 2 == 0), S=[140, 100], P=[5, 2])


def tail(D):
    """S - P + 1 = 8 for the first utterance: D - 1 = 5 below, 8 equal, 11 above it."""
    return make(2, 12, 5, D, 12, obs=True, S=[12, 9], P=[5, 5])


TAIL_DS = (6, 9, 12)
SWEEP_US = (5, 130)


def sweep_Ss(rows):
    """S - 1 transition rows = one chunk of the sweeps, one row more, two chunks and a row."""
    return sorted({rows + 1, rows + 2, 2 * rows + 2})


def sweep(U, S):
    return _case(EC.chunk(U, S), 6)


def mode(obs, terminal):
    return _case(EC.mode(obs, terminal), 5)


def degenerate(D):
    """S = P (every duration is 1), twice, and P = 1 (one position holds all S = 9 steps)."""
    return make(3, 9, 6, D, 9, obs=True, S=[6, 3, 9], P=[6, 3, 1])


DEGENERATE_DS = (4, 11)


def exponent():
    return _case(EC.exponent(), 16)


def value(name):
    return _case(EC.value(name), 32)


def larger():
    return make(2, 200, 80, 32, 200, obs=True)


def single_path(obs=False):
    """One live path per utterance, every other transition -inf: (case, durations (B,U))."""
    B, T, U, D = 3, 20, 6, 8
    rng = np.random.default_rng(77)
    c = make(B, T, U, D, 77, obs, S=[20, 13, 6], P=[6, 4, 6])
    lt = np.full_like(c["lt"], -np.inf)
    dur = np.zeros((B, U), np.int64)
    for b in range(B):
        S, P = int(c["S"][b]), int(c["P"][b])
        cuts = np.sort(rng.choice(np.arange(1, S), size=P - 1, replace=False))
        start = np.concatenate([[0], cuts, [S]]).astype(np.int64)
        dur[b, :P] = np.diff(start)
        for p in range(P):
            lt[b, start[p]:start[p + 1] - 1, p, 0] = c["lt"][b, start[p]:start[p + 1] - 1, p, 0]
            if p < P - 1:
                lt[b, start[p + 1] - 1, p, 1] = c["lt"][b, start[p + 1] - 1, p, 1]
        lt[b, S - 1, P - 1, 0] = c["lt"][b, S - 1, P - 1, 0]
    c["lt"] = lt
    return c, dur


def case_makers(rows, tile, sweep_rows):
    """name -> function making the case, for every shape the GPU tests compare with the reference;
    rows, tile: the duration launch's chunk depth and positions per workgroup
    (ssnt_duration_posterior_block of the A/B build); sweep_rows(U, obs): the chunk depth of its
    sweeps (ssnt_duration_posterior_sweep_rows)."""
    out = {f"lane-{U}": (lambda U=U: lane(U)) for U in LANE_US}
    for S in chunk_Ss(rows):
        out[f"chunk-{S}"] = lambda S=S: chunk(S, tile)
    for U in SWEEP_US:
        Ss = set()
        for obs in (False, True):
            Ss |= set(sweep_Ss(sweep_rows(U, obs)))
        for S in sorted(Ss):
            out[f"sweep-{U}-{S}"] = lambda U=U, S=S: sweep(U, S)
    for D in BIN_DS_SHORT + BIN_DS_LONG:
        out[f"bins-{D}"] = lambda D=D: bins(D)
    for D in TAIL_DS:
        out[f"tail-{D}"] = lambda D=D: tail(D)
    for obs in (False, True):
        for terminal in (False, True):
            out[f"mode-obs{int(obs)}-term{int(terminal)}"] = lambda obs=obs, terminal=terminal: mode(obs, terminal)
    for D in DEGENERATE_DS:
        out[f"degenerate-{D}"] = lambda D=D: degenerate(D)
    out["exponent"] = exponent
    for name in VC.TOLERANCE_CLASSES:
        out[f"value-{name}"] = lambda name=name: value(name)
    out["single-path"] = lambda: single_path(False)[0]
    out["single-path-obs"] = lambda: single_path(True)[0]
    out["larger"] = larger
    return out


def all_cases(rows, tile, sweep_rows):
    return {name: f() for name, f in case_makers(rows, tile, sweep_rows).items()}


def reference(c):
    return R.duration_posterior_batch(c["lt"], c["S"], c["P"], c["D"], c["lo"], c["terminal"])


def impossible(c):
    """(B,U,D) bool: the elements that are exact zeros whatever the inputs hold: bin 0, rows
    p >= P_b, every bin d > S_b - P_b + 1 (the tail too), and all of an utterance without a lattice."""
    B, T, U = c["lt"].shape[:3]
    D = c["D"]
    m = np.zeros((B, U, D), bool)
    m[:, :, 0] = True
    for b in range(B):
        S, P = int(c["S"][b]), int(c["P"][b])
        if not (1 <= P <= S <= T and P <= U):
            m[b] = True
            continue
        m[b, P:] = True
        m[b, :, min(S - P + 2, D):] = True
    return m


def errors(got, ref):
    """Worst error per output over the batch: absolute for dur_post (a probability); relative for
    loss (absolute where the reference is exactly 0; an infeasible utterance must be +inf on both
    sides)."""
    e = {"dur_post": float(np.max(np.abs(got["dur_post"].astype(np.float64) - ref["dur_post"]), initial=0.0))}
    gl, rl = got["loss"].astype(np.float64), ref["loss"]
    fin = np.isfinite(rl)
    assert np.array_equal(np.isposinf(gl), ~fin), (gl, rl)
    den = np.where(rl[fin] == 0, 1.0, np.abs(rl[fin]))
    e["loss"] = float(np.max(np.abs(gl[fin] - rl[fin]) / den, initial=0.0))
    return e
