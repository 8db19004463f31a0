"""References for the best-path (Viterbi) alignment on the emit/shift lattice.

``dp``: the specified recurrence in numpy float32, vectorised over positions and the batch --
the same IEEE adds and compares in the same order as the kernel, so the GPU must match it bit
for bit. ``brute_force``: every monotone path of one tiny utterance, each summed sequentially
in float32 (S-1 <= 10). Test infrastructure only."""
import itertools

import numpy as np

F32 = np.float32
NINF = F32(-np.inf)


def dp(lt, S, P, lo=None, terminal=True):
    """lt (B,T,U,2) f32, S / P (B,) ints, lo (B,T,U) f32 or None.
    Returns dict(log_prob (B,) f32, position (B,T) i32, duration (B,U) i32)."""
    lt = np.asarray(lt, F32)
    B, T, U, _ = lt.shape
    S = np.asarray(S, np.int64).reshape(B)
    P = np.asarray(P, np.int64).reshape(B)
    log_prob = np.full(B, NINF, F32)
    position = np.full((B, T), -1, np.int32)
    duration = np.zeros((B, U), np.int32)
    ok = (S >= 1) & (P >= 1) & (S <= T) & (P <= U) & (S >= P)
    if T == 0 or U == 0 or not ok.any():
        return {"log_prob": log_prob, "position": position, "duration": duration}
    V = np.full((B, U), NINF, F32)
    V[:, 0] = lo[:, 0, 0] if lo is not None else F32(0)
    bp = np.zeros((B, T, U), bool)
    final = np.full(B, NINF, F32)
    rows = np.arange(B)
    with np.errstate(invalid="ignore"):
        for s in range(T):
            if s > 0:
                stay = V + lt[:, s - 1, :, 0]
                move = np.full((B, U), NINF, F32)
                move[:, 1:] = V[:, :-1] + lt[:, s - 1, :-1, 1]
                bp[:, s] = move > stay  # strict: a tie keeps the emit
                V = np.where(bp[:, s], move, stay).astype(F32)
                if lo is not None:
                    V = V + lo[:, s]
            last = ok & (S - 1 == s)
            if last.any():
                final[last] = V[rows[last], P[last] - 1]
        for b in np.nonzero(ok)[0]:
            v = final[b]
            if terminal:
                v = F32(v + lt[b, S[b] - 1, P[b] - 1, 0])
            if not v > NINF:
                continue
            log_prob[b] = v
            p = P[b] - 1
            for s in range(S[b] - 1, -1, -1):
                position[b, s] = p
                duration[b, p] += 1
                if s > 0 and bp[b, s, p]:
                    p -= 1
            assert p == 0
    return {"log_prob": log_prob, "position": position, "duration": duration}


def brute_force(lt, S, P, lo=None, terminal=True):
    """One utterance: lt (T,U,2), lo (T,U) or None. The maximum over all monotone paths of the
    sequential float32 sum of each path. Returns (log_prob f32, list of the maximal paths, each
    a tuple of S positions)."""
    lt = np.asarray(lt, F32)
    T, U, _ = lt.shape
    if not (S >= 1 and P >= 1 and S <= T and P <= U and S >= P):
        return NINF, []
    assert S - 1 <= 10
    best, arg = NINF, []
    with np.errstate(invalid="ignore"):
        for moves in itertools.combinations(range(1, S), P - 1):  # the steps that shift
            mv = set(moves)
            v = lo[0, 0] if lo is not None else F32(0)
            p, path = 0, [0]
            for s in range(1, S):
                if s in mv:
                    v = F32(v + lt[s - 1, p, 1])
                    p += 1
                else:
                    v = F32(v + lt[s - 1, p, 0])
                if lo is not None:
                    v = F32(v + lo[s, p])
                path.append(p)
            if terminal:
                v = F32(v + lt[S - 1, P - 1, 0])
            if v > best:
                best, arg = v, [tuple(path)]
            elif v == best and v > NINF:
                arg.append(tuple(path))
    return best, arg
