"""References for the exact N-best alignments on the emit/shift lattice.

``dp``: the specified recurrence in numpy float32, vectorised over positions and the batch --
the same IEEE adds in the same order and the same total order (value descending, tag ascending)
as the kernel, so the GPU must match it bit for bit. ``brute_force``: every monotone path of one
tiny utterance with its sequential float32 sum (S-1 <= 10). ``path_log_prob_f32`` is
tests/sample_ref.py's. Test infrastructure only."""
import itertools

import numpy as np

from sample_ref import path_log_prob_f32  # noqa: F401  (re-exported for the tests)

F32 = np.float32
NINF = F32(-np.inf)


def dp(lt, S, P, N, lo=None, terminal=True):
    """lt (B,T,U,2) f32, S / P (B,) ints, N = num_best, lo (B,T,U) f32 or None.
    Returns dict(log_prob (B,N) f32, position (B,N,T) i32, duration (B,N,U) i32, count (B,) i32)."""
    lt = np.asarray(lt, F32)
    B, T, U, _ = lt.shape
    S = np.asarray(S, np.int64).reshape(B)
    P = np.asarray(P, np.int64).reshape(B)
    log_prob = np.full((B, N), NINF, F32)
    position = np.full((B, N, T), -1, np.int32)
    duration = np.zeros((B, N, U), np.int32)
    count = np.zeros(B, np.int32)
    res = {"log_prob": log_prob, "position": position, "duration": duration, "count": count}
    ok = (S >= 1) & (P >= 1) & (S <= T) & (P <= U) & (S >= P)
    if T == 0 or U == 0 or not ok.any():
        return res
    V = np.full((B, U, N), NINF, F32)
    V[:, 0, 0] = lo[:, 0, 0] if lo is not None else F32(0)
    bp = np.zeros((B, T, U, N), np.int8)
    final = np.full((B, N), NINF, F32)
    rows = np.arange(B)
    with np.errstate(invalid="ignore"):
        for s in range(T):
            if s > 0:
                cand = np.full((B, U, 2 * N), NINF, F32)  # index = tag: stay_r at r, move_r at N + r
                cand[:, :, :N] = V + lt[:, s - 1, :, 0, None]
                cand[:, 1:, N:] = V[:, :-1] + lt[:, s - 1, :-1, 1, None]
                # (value descending, tag ascending): a stable sort of the candidates in tag order
                order = np.argsort(-cand, axis=-1, kind="stable")[..., :N]
                V = np.take_along_axis(cand, order, axis=-1).astype(F32)
                bp[:, s] = order
                if lo is not None:
                    V = V + lo[:, s, :, None]
            last = ok & (S - 1 == s)
            if last.any():
                final[last] = V[rows[last], P[last] - 1]
        for b in np.nonzero(ok)[0]:
            for n in range(N):
                v = final[b, n]
                if terminal:
                    v = F32(v + lt[b, S[b] - 1, P[b] - 1, 0])
                if not v > NINF:
                    break  # the list is sorted: present ranks come first
                log_prob[b, n] = v
                count[b] += 1
                p, r = P[b] - 1, n
                for s in range(S[b] - 1, -1, -1):
                    position[b, n, s] = p
                    duration[b, n, p] += 1
                    if s > 0:
                        tag = int(bp[b, s, p, r])
                        p -= tag // N
                        r = tag % N
                assert p == 0 and r == 0
    return res


def brute_force(lt, S, P, lo=None, terminal=True):
    """One utterance: lt (T,U,2), lo (T,U) or None. Every monotone path with its sequential
    float32 sum: a list of (value f32, path as a tuple of S positions), in no particular order."""
    lt = np.asarray(lt, F32)
    T, U, _ = lt.shape
    if not (S >= 1 and P >= 1 and S <= T and P <= U and S >= P):
        return []
    assert S - 1 <= 10
    out = []
    with np.errstate(invalid="ignore"):
        for moves in itertools.combinations(range(1, S), P - 1):  # the steps that shift
            mv = set(moves)
            v = F32(lo[0, 0]) if lo is not None else F32(0)
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
            out.append((v, tuple(path)))
    return out


def top_values(paths, N):
    """The N largest values of brute_force's list, descending, padded with -inf; values that are
    not > -inf count as absent."""
    vals = sorted((float(v) for v, _ in paths if v > NINF), reverse=True)[:N]
    return np.array(vals + [-np.inf] * (N - len(vals)), F32)
