"""The best duration path on the v2 duration-class lattice, restated for the tests (DESIGN.md
2.3): `dp`, the recurrence in numpy float32 -- the definition the GPU kernel is bit-identical
to -- and `brute_force`, every class sequence of one tiny utterance.

dp is vectorised over the batch and the cells of a row; the classes are taken one after the
other in increasing order with the strict compare of the definition (`c > best`), so a tie keeps
the lower class and a NaN candidate never wins, exactly as the recurrence states it."""
import functools

import numpy as np

from f4_cases import band, move_ok, random_case

NINF = np.float32(-np.inf)


def window(r, I, O, X, dmax, test_mode):
    """Cells [lo, hi] of row r that can hold a path (empty when lo > hi); = F4's f4_window."""
    if r == 0:
        return 0, 0
    if test_mode:
        return 0, min(r * dmax, X - 1)
    t = r - 1
    if (I - (t + 1)) * 3 > O:
        return 1, 0
    lb, ub = band(t, I, O)
    if t == I - 1:
        lb, ub = max(lb, O), min(ub, O)
    return max(lb, 0), min(ub, X - 1)


def _empty(B, T):
    return {"log_prob": np.full(B, NINF, np.float32), "duration_class": np.full((B, T), -1, np.int32),
            "duration": np.zeros((B, T), np.int32), "total": np.full(B, -1, np.int32)}


def dp(logits, table, I, O, max_total, zid, allow_skip, test_mode):
    """log_prob (B,), duration_class (B,T), duration (B,T), total (B,) of the best path."""
    logits = np.asarray(logits, np.float32)
    table = np.asarray(table, np.int64)
    I = np.asarray(I, np.int64)
    O = np.asarray(O, np.int64)
    B, T, D = logits.shape
    X = int(max_total) + 1
    res = _empty(B, T)
    if (table < 0).any():
        return res
    dmax = int(table.max())
    ok = (I >= 1) & (I <= T) & (O >= 0)
    if not test_mode:
        ok &= O <= X - 1
    if not ok.any():
        return res
    Imax = int(I[ok].max())
    # windows of every (utterance, row)
    lo = np.ones((B, Imax + 1), np.int64)
    hi = np.zeros((B, Imax + 1), np.int64)
    for b in np.flatnonzero(ok):
        for r in range(int(I[b]) + 1):
            lo[b, r], hi[b, r] = window(r, int(I[b]), int(O[b]), X, dmax, test_mode)
    w = logits.copy()
    if not allow_skip:
        w[:, :, zid] = NINF
    pad = dmax
    cols = np.arange(X)
    V = np.full((B, pad + X), NINF, np.float32)  # V[b, pad + x]; the pad cells stay -inf
    V[ok, pad] = np.float32(0.0)
    bp = np.full((B, Imax, X), -1, np.int8)
    final = np.full((B, X), NINF, np.float32)
    with np.errstate(invalid="ignore"):
        for r in range(1, Imax + 1):
            act = ok & (I >= r)
            c0 = int(lo[act, r].min())
            c1 = int(hi[act, r].max())
            best = np.full((B, X), NINF, np.float32)
            arg = np.full((B, X), -1, np.int8)
            if c1 >= c0:
                sb, sa = best[:, c0:c1 + 1], arg[:, c0:c1 + 1]
                for i in range(D):  # increasing: a tie keeps the lower class
                    d = int(table[i])
                    c = V[:, pad + c0 - d:pad + c1 + 1 - d] + w[:, r - 1, i][:, None]
                    m = c > sb  # strict; False for a NaN
                    sb[m] = c[m]
                    sa[m] = i
            inw = act[:, None] & (cols[None, :] >= lo[:, r, None]) & (cols[None, :] <= hi[:, r, None])
            best[~inw] = NINF
            arg[~inw] = -1
            V[:, pad:] = best
            bp[:, r - 1] = arg
            done = ok & (I == r)
            final[done] = best[done]
    for b in np.flatnonzero(ok):
        row = final[b]
        m = row.max()
        if not m > NINF:
            continue
        x = int(np.flatnonzero(row == m)[0])  # a tie keeps the lowest total
        res["log_prob"][b] = m
        res["total"][b] = x
        for r in range(int(I[b]), 0, -1):
            i = int(bp[b, r - 1, x])
            assert i >= 0
            res["duration_class"][b, r - 1] = i
            res["duration"][b, r - 1] = table[i]
            x -= int(table[i])
        assert x == 0
    return res


def brute_force(logits, table, I, O, max_total, zid, allow_skip, test_mode):
    """Every class sequence of one utterance (logits (T,D)), in lexicographic order, cut at the
    first move f4_cases.move_ok refuses: the largest sequential f32 sum over the admissible ones
    and all sequences that attain it ([] when none is above -inf)."""
    D = logits.shape[1]
    X = max_total + 1
    state = {"best": NINF, "arg": []}

    def walk(t, tot, v, seq):
        if t == I:
            if v > state["best"]:
                state["best"], state["arg"] = v, [tuple(seq)]
            elif v == state["best"] and v > NINF:
                state["arg"].append(tuple(seq))
            return
        for i in range(D):
            nt = tot + int(table[i])
            if not move_ok(t, nt, i, I, O, X, zid, allow_skip, test_mode):
                continue
            with np.errstate(invalid="ignore"):
                nv = np.float32(v + logits[t, i])
            walk(t + 1, nt, nv, seq + [i])

    if I >= 1:
        walk(0, 0, np.float32(0.0), [])
    return state["best"], state["arg"]


# ---- the tiny cases both test files share (CPU: dp against brute force; GPU: the kernel) ------
TABLE4 = np.array([0, 1, 2, 3], np.int32)
TIE_TABLE = np.array([0, 1, 2, 1], np.int32)
MODES = ["band", "test_mode", "no_skip"]


def tiny_case(seed, mode):
    """B=12, Imax=6, D=4 from f4_cases.random_case; test mode leaves 3 totals above max O.
    Returns logits, table, I, O, max_total, allow_skip, test_mode."""
    logits, I, O = random_case(np.random.default_rng(seed), 12, 6, 4)
    test_mode, allow_skip = mode == "test_mode", mode != "no_skip"
    return logits, TABLE4, I, O, int(O.max()) + (3 if test_mode else 0), allow_skip, test_mode


def tie_case(seed, test_mode, B=10, Imax=5):
    """Logits from {-0.5, -1, -1.5} and two classes of duration 1: many sequences reach the same
    f32 sum. I in 2..Imax. Same return as tiny_case."""
    rng = np.random.default_rng(1000 + seed)
    logits = rng.choice(np.array([-0.5, -1.0, -1.5], np.float32), size=(B, Imax, len(TIE_TABLE)))
    I = rng.integers(2, Imax + 1, size=B).astype(np.int32)
    O = np.array([int(rng.integers(i, 2 * i + 1)) for i in I], np.int32)
    return logits, TIE_TABLE, I, O, int(O.max()) + (3 if test_mode else 0), True, bool(test_mode)


@functools.lru_cache(maxsize=None)
def case_brute_force(kind, seed, mode):
    """brute_force of every utterance of tiny_case(seed, mode) / tie_case(seed, mode), once."""
    logits, table, I, O, mt, allow_skip, test_mode = (tiny_case if kind == "tiny" else tie_case)(seed, mode)
    return [brute_force(logits[b], table, int(I[b]), int(O[b]), mt, 0, allow_skip, test_mode)
            for b in range(len(I))]


def check_against_brute_force(r, case, brute):
    """r (dp's or the GPU's outputs) against brute force: the value bit-equal, the path one of the
    maximal ones (the one when unique), sum(duration) == total, total == O in band mode.
    Returns the (feasible, tied) counts."""
    logits, table, I, O, mt, allow_skip, test_mode = case
    feasible = tied = 0
    for b, (best, arg) in enumerate(brute):
        assert r["log_prob"][b].tobytes() == np.float32(best).tobytes(), (b, r["log_prob"][b], best)
        if not arg:
            assert r["total"][b] == -1
            assert np.all(r["duration_class"][b] == -1) and np.all(r["duration"][b] == 0)
            continue
        feasible += 1
        tied += len(arg) > 1
        n = int(I[b])
        path = tuple(int(c) for c in r["duration_class"][b, :n])
        assert path in arg, (b, path, arg)
        assert np.all(r["duration_class"][b, n:] == -1) and np.all(r["duration"][b, n:] == 0)
        assert np.array_equal(r["duration"][b, :n], table[list(path)])
        assert int(r["duration"][b].sum()) == int(r["total"][b])
        if not test_mode:
            assert int(r["total"][b]) == int(O[b])
    return feasible, tied
