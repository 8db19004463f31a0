"""Float64 reference for the posterior duration distribution on the emit/shift lattice
(DESIGN.md 2.10).

``duration_posterior``: the formulas of section 2.10 as a numpy DP for one utterance, everything in
the log domain (no underflow at any size): alpha, beta, then for d = 1, 2, .. the vector over entry
steps s of ln(entry(s,p) * G(s,d)), closed with exit (an exact duration) or beta (the tail).
``brute_force``: every path of a tiny lattice with its posterior probability, the bins as plain
sums over paths. ``occupancy``: sum_s gamma[s,p], the mean duration. Test infrastructure only."""
import itertools

import numpy as np

from sample_ref import feasible_shape


def _lse0(x):
    """logsumexp over axis 0; a column of -inf gives -inf."""
    with np.errstate(invalid="ignore", divide="ignore"):
        m = x.max(axis=0)
        ms = np.where(np.isneginf(m), 0.0, m)
        return np.where(np.isneginf(m), -np.inf, ms + np.log(np.exp(x - ms).sum(axis=0)))


def log_alpha_beta(lt, S, P, lo=None, terminal=True):
    """(la, lb, e, sh, o, lnz) of the (S,P) lattice, float64, beta without O of its own cell."""
    lt = np.asarray(lt, np.float64)
    ninf = -np.inf
    o = np.zeros((S, P)) if lo is None else np.asarray(lo, np.float64)[:S, :P].copy()
    e = lt[:S, :P, 0].copy()
    sh = lt[:S, :P, 1].copy()
    sh[:, P - 1] = ninf
    sh[S - 1, :] = ninf
    term = e[S - 1, P - 1] if terminal else 0.0
    e[S - 1, :] = ninf  # (row S-1 has no emit but the terminal one)
    for a in (o, e, sh):
        a[np.isnan(a)] = ninf
    la = np.full((S, P), ninf)
    lb = np.full((S, P), ninf)
    la[0, 0] = o[0, 0]
    for s in range(1, S):
        move = np.full(P, ninf)
        move[1:] = la[s - 1, :-1] + sh[s - 1, :-1]
        la[s] = np.logaddexp(la[s - 1] + e[s - 1], move) + o[s]
    lb[S - 1, P - 1] = ninf if np.isnan(term) else term
    for s in range(S - 2, -1, -1):
        q = lb[s + 1] + o[s + 1]
        u2 = np.full(P, ninf)
        u2[:-1] = sh[s, :-1] + q[1:]
        lb[s] = np.logaddexp(e[s] + q, u2)
    return la, lb, e, sh, o, la[S - 1, P - 1] + lb[S - 1, P - 1]


def duration_posterior(lt, S, P, D, lo=None, terminal=True):
    """One utterance: lt (T,U,2), lo (T,U) or None, D bins. dict(feasible, dur_post (U,D), loss),
    float64, with the infeasible rule of 2.10."""
    T, U, _ = np.shape(lt)
    res = {"feasible": False, "dur_post": np.zeros((U, D)), "loss": np.inf}
    if not feasible_shape(S, P, T, U):
        return res
    ninf = -np.inf
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        la, lb, e, sh, o, lnz = log_alpha_beta(lt, S, P, lo, terminal)
        if not lnz > ninf:
            return res
        ent = np.full((S, P), ninf)
        ent[0, 0] = la[0, 0]
        ent[1:, 1:] = la[:-1, :-1] + sh[:-1, :-1] + o[1:, 1:]
        stay = np.full((S, P), ninf)
        stay[:-1] = e[:-1] + o[1:]
        ext = np.full((S, P), ninf)
        ext[:-1, :-1] = sh[:-1, :-1] + lb[1:, 1:] + o[1:, 1:]
        ext[S - 1, P - 1] = lb[S - 1, P - 1]
        dp = np.zeros((U, D))
        F = ent.copy()  # F[s] = ln(entry(s) * G(s, d)), rows s = 0 .. S-d
        for d in range(1, min(D - 1, S) + 1):
            close = lb if d == D - 1 else ext
            dp[:P, d] = np.exp(_lse0(F + close[d - 1:]) - lnz)
            F = F[:-1] + stay[d - 1:S - 1]
    res.update(feasible=True, dur_post=dp, loss=float(-lnz))
    return res


def duration_posterior_batch(lt, S, P, D, lo=None, terminal=True):
    """lt (B,T,U,2): the per-utterance results stacked."""
    rs = [duration_posterior(lt[b], int(S[b]), int(P[b]), D, None if lo is None else lo[b], terminal)
          for b in range(lt.shape[0])]
    return {k: np.stack([np.asarray(r[k]) for r in rs]) for k in rs[0]}


def occupancy(lt, S, P, lo=None, terminal=True):
    """(P,) sum over s of the cell posterior gamma[s,p] = alpha * beta / Z: the mean duration."""
    with np.errstate(invalid="ignore", divide="ignore"):
        la, lb, _, _, _, lnz = log_alpha_beta(lt, S, P, lo, terminal)
        g = np.exp(la + lb - lnz)
    return np.where(np.isnan(g), 0.0, g).sum(axis=0)


def brute_force(lt, S, P, D, lo=None, terminal=True):
    """Every monotone path of one tiny utterance (S - 1 <= 10): dict(dur_post (U,D), loss)."""
    lt = np.asarray(lt, np.float64)
    T, U, _ = lt.shape
    assert S - 1 <= 10 and S >= P >= 1
    durs, scores = [], []
    for moves in itertools.combinations(range(1, S), P - 1):  # the steps that shift
        mv = set(moves)
        sc = 0.0 if lo is None else float(lo[0, 0])
        p = 0
        for s in range(1, S):
            k = 1 if s in mv else 0
            sc += lt[s - 1, p, k]
            p += k
            if lo is not None:
                sc += float(lo[s, p])
        if terminal:
            sc += lt[S - 1, P - 1, 0]
        start = [0] + list(moves) + [S]
        durs.append(np.diff(start))
        scores.append(sc)
    scores = np.array(scores)
    m = scores.max()
    w = np.exp(scores - m)
    pr = w / w.sum()
    dp = np.zeros((U, D))
    for dur, q in zip(durs, pr):
        for p, d in enumerate(dur):
            dp[p, min(int(d), D - 1)] += q
    return {"dur_post": dp, "loss": float(-(m + np.log(w.sum())))}
