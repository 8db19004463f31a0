"""Float64 reference for posterior sampling on the emit/shift lattice.

``log_alpha``: the forward recurrence as a numpy log-domain DP. ``sample``: forward filter,
backward sample for one utterance, vectorised over its samples: rho[s][p] = P(move into (s,p)) =
exp(move - logaddexp(stay, move)); walking back from (S-1, P-1), sample k moves iff u[k,s] <
rho[s][p]. Each sample also gets its margin, min |u[s] - rho| over the visited cells with 0 < rho
< 1: a sample whose margin exceeds DELTA is *clear*, and an f32 implementation must reproduce its
path exactly (forced decisions, rho exactly 0 or 1, are exact on both sides and carry no margin).
``path_log_prob_f32`` restates the sequential f32 sum of a path; ``path_posterior`` enumerates
every path of a tiny lattice. Test infrastructure only."""
import itertools

import numpy as np

F32 = np.float32
DELTA = 1e-4
U_MAX = F32(1.0) - F32(2.0 ** -24)


def clamp_uniform(u):
    """The kernel's clamp, in f32: NaN -> 0, then [0, 1 - 2^-24]."""
    u = np.asarray(u, F32)
    u = np.where(u >= 0, u, F32(0))
    return np.minimum(u, U_MAX).astype(F32)


def feasible_shape(S, P, T, U):
    return S >= 1 and P >= 1 and S <= T and P <= U and S >= P


def log_alpha(lt, S, P, lo=None):
    """lt (T,U,2), lo (T,U) or None -> (la (S,P) f64, stay (S,P), move (S,P)): the two log terms
    entering every cell (row 0: -inf)."""
    lt = np.asarray(lt, np.float64)
    ninf = -np.inf
    la = np.full((S, P), ninf)
    stay = np.full((S, P), ninf)
    move = np.full((S, P), ninf)
    la[0, 0] = 0.0 if lo is None else float(lo[0, 0])
    with np.errstate(invalid="ignore"):
        for s in range(1, S):
            stay[s] = la[s - 1] + lt[s - 1, :P, 0]
            move[s, 1:] = la[s - 1, :-1] + lt[s - 1, :P - 1, 1]
            la[s] = np.logaddexp(stay[s], move[s])
            if lo is not None:
                la[s] = la[s] + np.asarray(lo[s, :P], np.float64)
    return la, stay, move


def move_prob(stay, move):
    """rho = exp(move - logaddexp(stay, move)); 0 where the cell is unreachable."""
    with np.errstate(invalid="ignore", divide="ignore"):
        tot = np.logaddexp(stay, move)
        rho = np.exp(move - tot)
    return np.where(np.isneginf(tot) | np.isneginf(move), 0.0, rho)


def sample(lt, S, P, u, lo=None):
    """One utterance: lt (T,U,2), u (K,T). Returns dict(feasible, position (K,T) i32, duration
    (K,U) i32, margin (K,) f64, rho (S,P))."""
    lt = np.asarray(lt, F32)
    T, U, _ = lt.shape
    u = clamp_uniform(u)
    K = u.shape[0]
    position = np.full((K, T), -1, np.int32)
    duration = np.zeros((K, U), np.int32)
    margin = np.full(K, np.inf)
    res = {"feasible": False, "position": position, "duration": duration, "margin": margin, "rho": None}
    if not feasible_shape(S, P, T, U):
        return res
    la, stay, move = log_alpha(lt, S, P, lo)
    if not la[S - 1, P - 1] > -np.inf:
        return res
    rho = move_prob(stay, move)
    res["feasible"], res["rho"] = True, rho
    p = np.full(K, P - 1, np.int64)
    for s in range(S - 1, 0, -1):
        position[:, s] = p
        r = rho[s, p]
        us = u[:, s].astype(np.float64)
        inner = (r > 0) & (r < 1)
        margin = np.where(inner, np.minimum(margin, np.abs(us - r)), margin)
        p = p - (us < r)
    assert np.all(p == 0)
    position[:, 0] = 0
    for k in range(K):
        duration[k] = np.bincount(position[k, :S], minlength=U)
    res["margin"] = margin
    return res


def sample_batch(lt, S, P, u, lo=None):
    """lt (B,T,U,2), u (B,K,T): the per-utterance results stacked."""
    B = lt.shape[0]
    rs = [sample(lt[b], int(S[b]), int(P[b]), u[b], None if lo is None else lo[b]) for b in range(B)]
    return {"feasible": np.array([r["feasible"] for r in rs]),
            "position": np.stack([r["position"] for r in rs]),
            "duration": np.stack([r["duration"] for r in rs]),
            "margin": np.stack([r["margin"] for r in rs])}


def clear(margin, feasible):
    """(B,K) bool: the samples an f32 implementation must reproduce exactly."""
    return (margin > DELTA) & np.asarray(feasible)[:, None]


def path_log_prob_f32(lt, lo, position, terminal):
    """The sequential f32 sum of DESIGN.md 2.4 along one path: lt (T,U,2), lo (T,U) or None,
    position (T,) with -1 beyond S."""
    lt = np.asarray(lt, F32)
    pos = np.asarray(position)
    S = int(np.sum(pos >= 0))
    if S == 0:
        return F32(-np.inf)
    v = F32(lo[0, 0]) if lo is not None else F32(0)
    with np.errstate(invalid="ignore"):
        for s in range(S - 1):
            v = F32(v + lt[s, pos[s], pos[s + 1] - pos[s]])
            if lo is not None:
                v = F32(v + F32(lo[s + 1, pos[s + 1]]))
        if terminal:
            v = F32(v + lt[S - 1, pos[S - 1], 0])
    return v


def path_posterior(lt, S, P, lo=None):
    """Every monotone path of one tiny utterance (S - 1 <= 10) with its posterior probability in
    float64: dict {tuple of S positions: probability}. (The terminal emit is common to all paths.)"""
    lt = np.asarray(lt, np.float64)
    assert S - 1 <= 10 and S >= P >= 1
    paths, scores = [], []
    for moves in itertools.combinations(range(1, S), P - 1):  # the steps that shift
        mv = set(moves)
        sc = 0.0 if lo is None else float(lo[0, 0])
        p, path = 0, [0]
        for s in range(1, S):
            k = 1 if s in mv else 0
            sc += lt[s - 1, p, k]
            p += k
            if lo is not None:
                sc += float(lo[s, p])
            path.append(p)
        paths.append(tuple(path))
        scores.append(sc)
    scores = np.array(scores)
    m = scores.max()
    w = np.exp(scores - m)
    w = w / w.sum()
    return dict(zip(paths, w))


def frequency_deviation(positions, S, post, floor=1e-3):
    """positions (N,T) drawn paths of one utterance; post from path_posterior. The largest
    |frequency - posterior| in binomial standard deviations over the paths with posterior >=
    floor."""
    N = positions.shape[0]
    keys, counts = np.unique(positions[:, :S], axis=0, return_counts=True)
    seen = {tuple(int(x) for x in k): int(c) for k, c in zip(keys, counts)}
    assert set(seen) <= set(post), "a drawn path is not a path of the lattice"
    worst = 0.0
    for path, q in post.items():
        if q < floor:
            continue
        if q == 1.0:  # the only path: every draw is it
            assert seen.get(path, 0) == N
            continue
        sd = np.sqrt(q * (1 - q) / N)
        worst = max(worst, abs(seen.get(path, 0) / N - q) / sd)
    return worst
