"""The exact N best duration paths on the v2 duration-class lattice, restated for the tests
(DESIGN.md 2.7): `dp`, the recurrence in numpy float32 -- the definition the GPU kernel is
bit-identical to -- and `all_paths`, every admissible class sequence of one tiny utterance with
its sequential f32 sum.

dp is vectorised over the batch and the cells of a row. A cell's candidates lie along one axis in
key order (class * N + predecessor rank); its list is N rounds of "take the first maximum, remove
it", which is the total order of the definition (value descending, key ascending) taken N times.
A NaN candidate never enters a list, as v2_viterbi_ref.dp's strict compare has it at N = 1."""
import functools

import numpy as np

import v2_viterbi_ref as VR
from f4_cases import move_ok

NINF = np.float32(-np.inf)
NS = (1, 2, 3, 4, 8)


def _empty(B, T, N):
    return {"log_prob": np.full((B, N), NINF, np.float32), "duration_class": np.full((B, N, T), -1, np.int32),
            "duration": np.zeros((B, N, T), np.int32), "total": np.full((B, N), -1, np.int32),
            "count": np.zeros(B, np.int32)}


def _take_first_max(cand, axis):
    """The first maximum along `axis` (the lowest key among equal values): its index and value;
    it is removed from cand (set to -inf)."""
    idx = np.expand_dims(cand.argmax(axis=axis), axis)
    val = np.take_along_axis(cand, idx, axis)
    np.put_along_axis(cand, idx, NINF, axis)
    return np.squeeze(idx, axis), np.squeeze(val, axis)


def dp(logits, table, I, O, max_total, zid, allow_skip, test_mode, N):
    """log_prob (B,N), duration_class (B,N,T), duration (B,N,T), total (B,N), count (B,)."""
    logits = np.asarray(logits, np.float32)
    table = np.asarray(table, np.int64)
    I = np.asarray(I, np.int64)
    O = np.asarray(O, np.int64)
    B, T, D = logits.shape
    X = int(max_total) + 1
    res = _empty(B, T, N)
    if (table < 0).any():
        return res
    dmax = int(table.max())
    ok = (I >= 1) & (I <= T) & (O >= 0)
    if not test_mode:
        ok &= O <= X - 1
    if not ok.any():
        return res
    Imax = int(I[ok].max())
    lo = np.ones((B, Imax + 1), np.int64)
    hi = np.zeros((B, Imax + 1), np.int64)
    for b in np.flatnonzero(ok):
        for r in range(int(I[b]) + 1):
            lo[b, r], hi[b, r] = VR.window(r, int(I[b]), int(O[b]), X, dmax, test_mode)
    w = logits.copy()
    if not allow_skip:
        w[:, :, zid] = NINF
    pad = dmax
    cols = np.arange(X)
    V = np.full((B, N, pad + X), NINF, np.float32)  # V[b, rank, pad + x]; the pad cells stay -inf
    V[ok, 0, pad] = np.float32(0.0)
    bp = np.zeros((B, Imax, N, X), np.int16)  # class * N + predecessor rank
    final = np.full((B, N, X), NINF, np.float32)
    with np.errstate(invalid="ignore"):
        for r in range(1, Imax + 1):
            act = ok & (I >= r)
            c0 = int(lo[act, r].min())
            c1 = int(hi[act, r].max())
            best = np.full((B, N, X), NINF, np.float32)
            arg = np.zeros((B, N, X), np.int16)
            if c1 >= c0:
                cand = np.empty((B, D * N, c1 - c0 + 1), np.float32)
                for i in range(D):
                    d = int(table[i])
                    cand[:, i * N:(i + 1) * N] = V[:, :, pad + c0 - d:pad + c1 + 1 - d] + w[:, r - 1, i][:, None, None]
                cand[np.isnan(cand)] = NINF
                for n in range(N):
                    arg[:, n, c0:c1 + 1], best[:, n, c0:c1 + 1] = _take_first_max(cand, 1)
            inw = act[:, None] & (cols[None, :] >= lo[:, r, None]) & (cols[None, :] <= hi[:, r, None])
            best = np.where(inw[:, None, :], best, NINF)
            V[:, :, pad:] = best
            bp[:, r - 1] = arg
            done = ok & (I == r)
            final[done] = best[done]
    for b in np.flatnonzero(ok):
        cand = np.ascontiguousarray(final[b].T).reshape(-1)  # key order: total * N + rank
        for n in range(N):
            key, v = _take_first_max(cand, 0)
            if not v > NINF:
                break  # the order is total: present ranks come first
            x, q = int(key) // N, int(key) % N
            res["log_prob"][b, n] = v
            res["total"][b, n] = x
            res["count"][b] += 1
            for r in range(int(I[b]), 0, -1):
                i, q = divmod(int(bp[b, r - 1, q, x]), N)
                res["duration_class"][b, n, r - 1] = i
                res["duration"][b, n, r - 1] = table[i]
                x -= int(table[i])
            assert x == 0 and q == 0
    return res


def all_paths(logits, table, I, O, max_total, zid, allow_skip, test_mode):
    """Every class sequence of one utterance (logits (T,D)) that f4_cases.move_ok admits move by
    move, with its sequential f32 sum from 0.0f: a list of (value, sequence)."""
    D = logits.shape[1]
    X = max_total + 1
    out = []

    def walk(t, tot, v, seq):
        if t == I:
            out.append((v, tuple(seq)))
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
    return out


# ---- the case families both test files share ---------------------------------------------------
WIDE_TABLE = np.array([0, 2, 3, 4, 5, 7], np.int32)
WIDE_SEEDS = tuple(range(2000, 2006))


def wide_case(seed, allow_skip):
    """Band mode with room for 8 paths (tiny_case's band rarely has them): B=12, I in 3..6, O in
    [3 I, 5 I], softmaxed N(0, 1.5^2) logits. Same return as v2_viterbi_ref.tiny_case."""
    rng = np.random.default_rng(seed)
    B, Imax, D = 12, 6, len(WIDE_TABLE)
    I = rng.integers(3, Imax + 1, size=B).astype(np.int32)
    O = np.array([int(rng.integers(3 * i, 5 * i + 1)) for i in I], np.int32)
    z = rng.standard_normal((B, Imax, D)).astype(np.float32) * np.float32(1.5)
    m = z.max(-1, keepdims=True)
    logits = (z - (m + np.log(np.exp(z - m).sum(-1, keepdims=True)))).astype(np.float32)
    return logits, WIDE_TABLE, I, O, int(O.max()), bool(allow_skip), False


def family(kind):
    """(seed, mode) of every case of a family: "tiny", "tie" or "wide"."""
    if kind == "tiny":
        return [(s, m) for m in VR.MODES for s in range(6)]
    if kind == "tie":
        return [(s, tm) for tm in (False, True) for s in range(6)]
    return [(s, sk) for sk in (True, False) for s in WIDE_SEEDS]


def case(kind, seed, mode):
    return {"tiny": VR.tiny_case, "tie": VR.tie_case, "wide": wide_case}[kind](seed, mode)


@functools.lru_cache(maxsize=None)
def case_paths(kind, seed, mode):
    """all_paths of every utterance of case(kind, seed, mode), once."""
    logits, table, I, O, mt, allow_skip, test_mode = case(kind, seed, mode)
    return [all_paths(logits[b], table, int(I[b]), int(O[b]), mt, 0, allow_skip, test_mode)
            for b in range(len(I))]


def check_against_paths(r, cs, paths, N):
    """r (dp's or the GPU's outputs at num_best N) against the enumeration: the values bit-equal to
    the N largest sums, each path among the enumerated ones that carry its value, the paths
    pairwise distinct, each re-summing exactly, absent ranks by the rule, count right.
    Returns the number of admissible sequences with positive probability per utterance."""
    logits, table, I, O, mt, allow_skip, test_mode = cs
    finite = []
    for b, plist in enumerate(paths):
        value_of = {seq: v for v, seq in plist if v > NINF}
        finite.append(len(value_of))
        vals = sorted((float(v) for v in value_of.values()), reverse=True)[:N]
        n = len(vals)
        top = np.array(vals + [-np.inf] * (N - n), np.float32)
        assert r["log_prob"][b].tobytes() == top.tobytes(), (b, N, r["log_prob"][b], top)
        assert int(r["count"][b]) == n, (b, N)
        assert np.all(r["total"][b, n:] == -1), (b, N)
        assert np.all(r["duration_class"][b, n:] == -1) and np.all(r["duration"][b, n:] == 0), (b, N)
        L = int(I[b])
        seen = set()
        for k in range(n):
            seq = tuple(int(c) for c in r["duration_class"][b, k, :L])
            assert seq not in seen, (b, N, k)
            seen.add(seq)
            assert seq in value_of, (b, N, k, seq)
            assert np.float32(value_of[seq]).tobytes() == r["log_prob"][b, k].tobytes(), (b, N, k)
            v = np.float32(0.0)
            for t, c in enumerate(seq):
                v = np.float32(v + logits[b, t, c])
            assert v.tobytes() == r["log_prob"][b, k].tobytes(), (b, N, k)
            assert np.all(r["duration_class"][b, k, L:] == -1) and np.all(r["duration"][b, k, L:] == 0)
            assert np.array_equal(r["duration"][b, k, :L], table[list(seq)])
            assert int(r["duration"][b, k].sum()) == int(r["total"][b, k])
            if not test_mode:
                assert int(r["total"][b, k]) == int(O[b])
    return finite
