"""Float64 reference for the expected path cost on the emit/shift lattice and its gradients
(DESIGN.md 2.8).

``expected_cost``: the forward / backward means of section 2.8 as a numpy DP for one utterance,
alpha and beta in the log domain (no underflow at any size), the means as convex combinations with
weights exp(term - logaddexp). ``brute_force``: every path of a tiny lattice (S - 1 <= 10) with its
posterior probability; risk, the three gradients and the entropy as plain sums over paths.
``torch_double_backward``: risk = sum_e cost_e * d lnZ / d log_trans_e through a linear-domain
torch DP, and its gradients by a second backward. ``live_edges`` / ``scale``: the edges inside the
lattice and the bound on any path's |cost| the tests normalise errors by. Test infrastructure
only."""
import itertools

import numpy as np

from sample_ref import feasible_shape


def live_edges(shape, S, P, terminal):
    """(T,U,2) bool: the edges a path of the (S,P) lattice can take (the terminal emit under the
    flag); the complement of contract_cases.lattice_dead_mask for log_trans."""
    T, U = shape[:2]
    m = np.zeros((T, U, 2), bool)
    if not feasible_shape(S, P, T, U):
        return m
    m[:S - 1, :P, 0] = True
    m[:S - 1, :P - 1, 1] = True
    if terminal:
        m[S - 1, P - 1, 0] = True
    return m


def scale(cost, S, P, terminal):
    """sum over steps s < S of max |cost[s]| over the live edges of the step; 1 where that is 0."""
    cost = np.asarray(cost, np.float64)
    m = live_edges(cost.shape, S, P, terminal)
    v = float(np.where(m, np.abs(np.where(m, cost, 0.0)), 0.0).max(axis=(1, 2)).sum())
    return v if v > 0 else 1.0


def _wmean(l1, x1, l2, x2):
    """(w1*x1 + w2*x2) with w = exp(l - logaddexp(l1, l2)); a -inf term contributes an exact 0
    whatever its x holds, and no term at all gives 0. Returns (logaddexp, mean)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        tot = np.logaddexp(l1, l2)
        w1 = np.where(np.isneginf(l1), 0.0, np.exp(l1 - tot))
        w2 = np.where(np.isneginf(l2), 0.0, np.exp(l2 - tot))
        mean = np.where(w1 > 0, w1 * np.where(w1 > 0, x1, 0.0), 0.0) + \
            np.where(w2 > 0, w2 * np.where(w2 > 0, x2, 0.0), 0.0)
    return tot, np.where(np.isneginf(tot), 0.0, mean)


def expected_cost(lt, cost, S, P, lo=None, terminal=True):
    """One utterance: lt, cost (T,U,2), lo (T,U) or None. dict(feasible, risk, loss, grad_trans
    (T,U,2), grad_cost (T,U,2), grad_obs (T,U)), float64, with the infeasible rule of 2.8."""
    lt = np.asarray(lt, np.float64)
    c = np.asarray(cost, np.float64)
    T, U, _ = lt.shape
    res = {"feasible": False, "risk": 0.0, "loss": np.inf, "grad_trans": np.zeros((T, U, 2)),
           "grad_cost": np.zeros((T, U, 2)), "grad_obs": np.zeros((T, U))}
    if not feasible_shape(S, P, T, U):
        return res
    ninf = -np.inf
    o = np.zeros((S, P)) if lo is None else np.asarray(lo, np.float64)[:S, :P]
    e = lt[:S, :P, 0]
    sh = lt[:S, :P, 1].copy()
    sh[:, P - 1] = ninf
    c0 = np.where(np.isfinite(c[:S, :P, 0]), c[:S, :P, 0], 0.0)  # (dead cells may hold anything)
    c1 = np.where(np.isfinite(c[:S, :P, 1]), c[:S, :P, 1], 0.0)
    la = np.full((S, P), ninf)
    ab = np.zeros((S, P))
    la[0, 0] = o[0, 0]
    with np.errstate(invalid="ignore"):
        for s in range(1, S):
            stay = la[s - 1] + e[s - 1]
            xs = ab[s - 1] + c0[s - 1]
            move = np.full(P, ninf)
            xm = np.zeros(P)
            move[1:] = la[s - 1, :-1] + sh[s - 1, :-1]
            xm[1:] = ab[s - 1, :-1] + c1[s - 1, :-1]
            tot, ab[s] = _wmean(stay, xs, move, xm)
            la[s] = tot + o[s]
        lb = np.full((S, P), ninf)
        bb = np.zeros((S, P))
        lb[S - 1, P - 1] = e[S - 1, P - 1] if terminal else 0.0
        bb[S - 1, P - 1] = c0[S - 1, P - 1] if terminal else 0.0
        for s in range(S - 2, -1, -1):
            q = lb[s + 1] + o[s + 1]
            u1 = e[s] + q
            x1 = c0[s] + bb[s + 1]
            u2 = np.full(P, ninf)
            x2 = np.zeros(P)
            u2[:-1] = sh[s, :-1] + q[1:]
            x2[:-1] = c1[s, :-1] + bb[s + 1, 1:]
            lb[s], bb[s] = _wmean(u1, x1, u2, x2)
        lnz = la[S - 1, P - 1] + lb[S - 1, P - 1]
        if not lnz > ninf:
            return res
        risk = ab[S - 1, P - 1] + bb[S - 1, P - 1]
        gt = np.zeros((T, U, 2))
        gc = np.zeros((T, U, 2))
        go = np.zeros((T, U))
        q = lb[1:] + o[1:]  # Q[s+1]
        q0 = np.exp(la[:-1] + e[:-1] + q - lnz)
        q0 = np.where(np.isnan(q0), 0.0, q0)
        gc[:S - 1, :P, 0] = q0
        gt[:S - 1, :P, 0] = np.where(q0 > 0, q0 * (ab[:-1] + c0[:-1] + bb[1:] - risk), 0.0)
        if P > 1:
            q1 = np.exp(la[:-1, :-1] + sh[:-1, :-1] + q[:, 1:] - lnz)
            q1 = np.where(np.isnan(q1), 0.0, q1)
            gc[:S - 1, :P - 1, 1] = q1
            gt[:S - 1, :P - 1, 1] = np.where(q1 > 0, q1 * (ab[:-1, :-1] + c1[:-1, :-1] + bb[1:, 1:] - risk), 0.0)
        if terminal:
            gc[S - 1, P - 1, 0] = 1.0
        post = np.exp(la + lb - lnz)  # (without log_obs: the derivative at log_obs = 0)
        post = np.where(np.isnan(post), 0.0, post)
        go[:S, :P] = np.where(post > 0, post * (ab + bb - risk), 0.0)
        go[S - 1] = 0.0  # (S-1, P-1) is on every path: exactly 0
    res.update(feasible=True, risk=float(risk), loss=float(-lnz), grad_trans=gt, grad_cost=gc, grad_obs=go)
    return res


def expected_cost_batch(lt, cost, S, P, lo=None, terminal=True):
    """lt, cost (B,T,U,2): the per-utterance results stacked (grad_obs only with lo)."""
    B = lt.shape[0]
    rs = [expected_cost(lt[b], cost[b], int(S[b]), int(P[b]), None if lo is None else lo[b], terminal)
          for b in range(B)]
    out = {k: np.stack([np.asarray(r[k]) for r in rs]) for k in rs[0]}
    out["scale"] = np.array([scale(cost[b], int(S[b]), int(P[b]), terminal) for b in range(B)])
    if lo is None:
        del out["grad_obs"]
    return out


def entropy_cost(lt, S, lo=None):
    """The cost whose risk is E[ln w(path)] - log_obs[0,0]: log_trans, plus the log_obs of the
    entered cell on both edges that enter it (rows s < S-1). lt (T,U,2) -> (T,U,2) float64."""
    c = np.array(lt, np.float64)
    if lo is not None:
        lo = np.asarray(lo, np.float64)
        c[:S - 1, :, 0] += lo[1:S]
        c[:S - 1, :-1, 1] += lo[1:S, 1:]
    return c


def brute_force(lt, cost, S, P, lo=None, terminal=True):
    """Every monotone path of one tiny utterance (S - 1 <= 10). dict as expected_cost plus
    ``entropy`` = -sum p ln p over the paths."""
    lt = np.asarray(lt, np.float64)
    c = np.asarray(cost, np.float64)
    T, U, _ = lt.shape
    assert S - 1 <= 10 and S >= P >= 1
    paths, scores, costs = [], [], []
    for moves in itertools.combinations(range(1, S), P - 1):  # the steps that shift
        mv = set(moves)
        sc = 0.0 if lo is None else float(lo[0, 0])
        cc, p, edges, cells = 0.0, 0, [], [(0, 0)]
        for s in range(1, S):
            k = 1 if s in mv else 0
            sc += lt[s - 1, p, k]
            cc += c[s - 1, p, k]
            edges.append((s - 1, p, k))
            p += k
            if lo is not None:
                sc += float(lo[s, p])
            cells.append((s, p))
        if terminal:
            sc += lt[S - 1, P - 1, 0]
            cc += c[S - 1, P - 1, 0]
            edges.append((S - 1, P - 1, 0))
        paths.append((edges, cells))
        scores.append(sc)
        costs.append(cc)
    scores, costs = np.array(scores), np.array(costs)
    m = scores.max()
    w = np.exp(scores - m)
    z = w.sum()
    pr = w / z
    risk = float((pr * costs).sum())
    gt, gc, go = np.zeros((T, U, 2)), np.zeros((T, U, 2)), np.zeros((T, U))
    for (edges, cells), q, cc in zip(paths, pr, costs):
        for ed in edges:
            gc[ed] += q
            gt[ed] += q * (cc - risk)
        for cell in cells:
            go[cell] += q * (cc - risk)
    nz = pr > 0
    return {"risk": risk, "loss": float(-(m + np.log(z))), "grad_trans": gt, "grad_cost": gc,
            "grad_obs": go, "entropy": float(-(pr[nz] * np.log(pr[nz])).sum())}


def torch_double_backward(lt, cost, S, P, lo=None, terminal=True):
    """risk and its gradients by autograd through a linear-domain float64 DP: risk =
    sum_e cost_e * d lnZ / d lt_e (first backward, create_graph), then d risk / d (lt, cost, lo)."""
    import torch
    lt_t = torch.tensor(np.asarray(lt, np.float64), requires_grad=True)
    c_t = torch.tensor(np.asarray(cost, np.float64), requires_grad=True)
    lo_t = None if lo is None else torch.tensor(np.asarray(lo, np.float64), requires_grad=True)
    w = torch.exp(lt_t)
    ob = None if lo_t is None else torch.exp(lo_t)
    alpha = [torch.zeros((), dtype=torch.float64) for _ in range(P)]
    alpha[0] = torch.ones((), dtype=torch.float64) if ob is None else ob[0, 0]
    for s in range(1, S):
        new = []
        for p in range(P):
            v = alpha[p] * w[s - 1, p, 0]
            if p > 0:
                v = v + alpha[p - 1] * w[s - 1, p - 1, 1]
            if ob is not None:
                v = v * ob[s, p]
            new.append(v)
        alpha = new
    z = alpha[P - 1] * (w[S - 1, P - 1, 0] if terminal else 1.0)
    lnz = torch.log(z)
    (dlt,) = torch.autograd.grad(lnz, lt_t, create_graph=True)
    risk = (dlt * c_t).sum()
    ins = [lt_t, c_t] + ([] if lo_t is None else [lo_t])
    gs = torch.autograd.grad(risk, ins, allow_unused=True)
    out = {"risk": float(risk.detach()), "loss": float(-lnz.detach()), "grad_trans": gs[0].numpy(), "grad_cost": gs[1].numpy()}
    if lo_t is not None:
        out["grad_obs"] = gs[2].numpy()
    return out
