"""Float64 reference for the expected path cost on the v2 duration-class lattice and its gradients
(DESIGN.md 2.9).

``expected_cost``: the forward / backward means of section 2.9 as a numpy DP for one utterance over
F4's lattice (f4_cases.band / move_ok restated per step as masks over the new total), alpha and
beta in the log domain (no underflow at any size), the means as convex combinations with weights
exp(term - logsumexp). ``brute_force``: every class sequence of a tiny utterance (D^I of them) with
its posterior probability; risk, both gradients and the entropy as plain sums over paths.
``torch_double_backward``: risk = sum cost * d lnZ / d logits through a linear-domain torch DP, and
its gradients by a second backward. ``allowed_classes`` / ``scale``: the classes a step can take
and the bound on any path's |cost| the tests normalise errors by. Test infrastructure only."""
import itertools

import numpy as np

from f4_cases import band, move_ok

LOG_MIN = -1.0e6  # log-probs below this (and NaN) are exact zeros, as the kernels' exp


def _clean_logits(logits):
    lg = np.asarray(logits, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(lg >= LOG_MIN, lg, -np.inf)


def allowed_classes(logits, zid, allow_skip):
    """(Imax, D) bool: the classes of weight non-zero that the class rule admits."""
    ok = ~np.isneginf(_clean_logits(logits))
    if not allow_skip and 0 <= zid < ok.shape[1]:
        ok = ok.copy()
        ok[:, zid] = False
    return ok


def feasible_lengths(I, O, Imax, table):
    return 1 <= I <= Imax and O >= 0 and not (np.asarray(table) < 0).any()


def scale(logits, cost, I, zid, allow_skip):
    """sum over steps t < I of max |cost[t]| over the allowed classes of the step; 1 where 0."""
    ok = allowed_classes(logits, zid, allow_skip)
    I = max(0, min(int(I), ok.shape[0]))
    c = np.where(ok, np.abs(np.where(ok, np.asarray(cost, np.float64), 0.0)), 0.0)
    v = float(c[:I].max(axis=1).sum()) if I > 0 else 0.0
    return v if v > 0 else 1.0


def _step_masks(t, I, O, X, test_mode):
    """(X,) bool over the new total nt of a move at step t: move_ok without its class rule."""
    nt = np.arange(X)
    if test_mode:
        return np.ones(X, bool)
    lb, ub = band(t, I, O)
    m = (nt >= lb) & (nt <= ub)
    if (I - (t + 1)) * 3 > O:
        m[:] = False
    if t == I - 1:
        m &= nt == O
    return m


def _lse_mean(terms, xs):
    """terms, xs (D, X): logsumexp over axis 0 and the convex combination of xs with weights
    exp(term - lse); a -inf term contributes an exact 0 whatever its x holds; no term: 0."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = terms.max(axis=0)
        ms = np.where(np.isfinite(m), m, 0.0)
        w = np.exp(terms - ms)
        w = np.where(np.isneginf(terms), 0.0, w)
        s = w.sum(axis=0)
        tot = np.where(s > 0, ms + np.log(np.where(s > 0, s, 1.0)), -np.inf)
        num = np.where(w > 0, w * np.where(w > 0, xs, 0.0), 0.0).sum(axis=0)
        mean = np.where(s > 0, num / np.where(s > 0, s, 1.0), 0.0)
    return tot, mean


def expected_cost(logits, cost, table, I, O, max_total, zid, allow_skip, test_mode):
    """One utterance: logits, cost (Imax, D). dict(feasible, risk, loss, grad_logits (Imax, D),
    grad_cost (Imax, D)), float64, with the no-admissible-path rule of 2.9."""
    Imax, D = np.asarray(logits).shape
    X = int(max_total) + 1
    res = {"feasible": False, "risk": 0.0, "loss": np.inf, "grad_logits": np.zeros((Imax, D)),
           "grad_cost": np.zeros((Imax, D))}
    I, O = int(I), int(O)
    table = np.asarray(table, np.int64)
    if not feasible_lengths(I, O, Imax, table):
        return res
    lg = _clean_logits(logits)
    cls_ok = allowed_classes(logits, zid, allow_skip)
    lg = np.where(cls_ok, lg, -np.inf)
    c = np.where(cls_ok, np.asarray(cost, np.float64), 0.0)  # (a dead class may hold anything)
    nt = np.arange(X)[None, :]
    src = nt - table[:, None]                 # (D, X): the source total of a move into nt
    src_ok = src >= 0
    srcc = np.clip(src, 0, X - 1)
    ninf = -np.inf
    la = np.full((I + 1, X), ninf)
    ab = np.zeros((I + 1, X))
    la[0, 0] = 0.0
    masks = [src_ok & _step_masks(t, I, O, X, test_mode)[None, :] for t in range(I)]
    with np.errstate(invalid="ignore"):
        for t in range(I):
            terms = np.where(masks[t], la[t][srcc] + lg[t][:, None], ninf)
            xs = ab[t][srcc] + c[t][:, None]
            la[t + 1], ab[t + 1] = _lse_mean(terms, xs)
        lb = np.full((I + 1, X), ninf)
        bb = np.zeros((I + 1, X))
        lb[I] = 0.0  # (band mode: the last step's mask admits the total O alone)
        for t in range(I - 1, -1, -1):
            # by destination nt, scattered to the source x = nt - d_i (one destination per class)
            terms_nt = np.where(masks[t], lg[t][:, None] + lb[t + 1][None, :], ninf)
            xs_nt = c[t][:, None] + bb[t + 1][None, :]
            terms = np.full((D, X), ninf)
            xs = np.zeros((D, X))
            for i in range(D):
                ok = masks[t][i]
                terms[i, srcc[i][ok]] = terms_nt[i][ok]
                xs[i, srcc[i][ok]] = xs_nt[i][ok]
            lb[t], bb[t] = _lse_mean(terms, xs)
        fin = la[I]
        m = fin.max()
        if not m > ninf:
            return res
        lnz = m + np.log(np.exp(fin - m).sum())
        pw = np.exp(fin - lnz)
        risk = float(np.where(pw > 0, pw * ab[I], 0.0).sum())
        gl = np.zeros((Imax, D))
        gc = np.zeros((Imax, D))
        for t in range(I):
            lq = np.where(masks[t], la[t][srcc] + lg[t][:, None] + lb[t + 1][None, :] - lnz, ninf)
            q = np.where(np.isneginf(lq) | np.isnan(lq), 0.0, np.exp(lq))
            dev = ab[t][srcc] + c[t][:, None] + bb[t + 1][None, :] - risk
            gc[t] = q.sum(axis=1)
            gl[t] = np.where(q > 0, q * np.where(q > 0, dev, 0.0), 0.0).sum(axis=1)
    res.update(feasible=True, risk=risk, loss=float(-lnz), grad_logits=gl, grad_cost=gc)
    return res


def expected_cost_batch(logits, cost, table, I, O, max_total, zid, allow_skip, test_mode):
    """logits, cost (B, Imax, D): the per-utterance results stacked, plus ``scale`` (B,)."""
    B = logits.shape[0]
    rs = [expected_cost(logits[b], cost[b], table, int(I[b]), int(O[b]), max_total, zid, allow_skip,
                        test_mode) for b in range(B)]
    out = {k: np.stack([np.asarray(r[k]) for r in rs]) for k in rs[0]}
    out["scale"] = np.array([scale(logits[b], cost[b], int(I[b]), zid, allow_skip) for b in range(B)])
    return out


def brute_force(logits, cost, table, I, O, max_total, zid, allow_skip, test_mode):
    """Every class sequence of one tiny utterance (f4_cases.brute_force's walk): dict as
    expected_cost plus ``entropy`` = -sum p ln p over the admissible sequences."""
    Imax, D = logits.shape
    X = max_total + 1
    res = {"feasible": False, "risk": 0.0, "loss": np.inf, "grad_logits": np.zeros((Imax, D)),
           "grad_cost": np.zeros((Imax, D)), "entropy": -np.inf}
    if not feasible_lengths(I, O, Imax, table):
        return res
    seqs, lps, ccs = [], [], []
    for seq in itertools.product(range(D), repeat=I):
        tot, ok, lp, cc = 0, True, 0.0, 0.0
        for t, i in enumerate(seq):
            tot += int(table[i])
            if not move_ok(t, tot, i, I, O, X, zid, allow_skip, test_mode) or not logits[t, i] >= LOG_MIN:
                ok = False
                break
            lp += float(logits[t, i])
            cc += float(cost[t, i])
        if ok:
            seqs.append(seq)
            lps.append(lp)
            ccs.append(cc)
    if not seqs:
        return res
    lps, ccs = np.array(lps), np.array(ccs)
    m = lps.max()
    w = np.exp(lps - m)
    z = w.sum()
    pr = w / z
    risk = float((pr * ccs).sum())
    gl, gc = np.zeros((Imax, D)), np.zeros((Imax, D))
    for seq, q, cc in zip(seqs, pr, ccs):
        for t, i in enumerate(seq):
            gc[t, i] += q
            gl[t, i] += q * (cc - risk)
    nz = pr > 0
    res.update(feasible=True, risk=risk, loss=float(-(m + np.log(z))), grad_logits=gl, grad_cost=gc,
               entropy=float(-(pr[nz] * np.log(pr[nz])).sum()))
    return res


def torch_double_backward(logits, cost, table, I, O, max_total, zid, allow_skip, test_mode):
    """risk and its gradients by autograd through a linear-domain float64 DP: risk =
    sum cost * d lnZ / d logits (first backward, create_graph), then d risk / d (logits, cost).
    Feasible utterances only; cost must be finite."""
    import torch
    Imax, D = logits.shape
    X = max_total + 1
    lg_t = torch.tensor(np.asarray(logits, np.float64), requires_grad=True)
    c_t = torch.tensor(np.asarray(cost, np.float64), requires_grad=True)
    w = torch.exp(lg_t)
    alpha = torch.zeros(X, dtype=torch.float64)
    alpha[0] = 1.0
    for t in range(I):
        new = torch.zeros(X, dtype=torch.float64)
        step = _step_masks(t, I, O, X, test_mode)
        for i in range(D):
            d = int(table[i])
            if (not allow_skip and i == zid) or d >= X or not logits[t, i] >= LOG_MIN:
                continue
            m = torch.tensor(step[d:])
            new = new + torch.cat([torch.zeros(d, dtype=torch.float64), alpha[:X - d] * w[t, i] * m])
        alpha = new
    z = alpha.sum()  # (band mode: the last step's mask admits the total O alone)
    lnz = torch.log(z)
    (dlg,) = torch.autograd.grad(lnz, lg_t, create_graph=True)
    risk = (dlg * c_t).sum()
    gs = torch.autograd.grad(risk, [lg_t, c_t])
    return {"risk": float(risk.detach()), "loss": float(-lnz.detach()), "grad_logits": gs[0].numpy(),
            "grad_cost": gs[1].numpy()}


def entropy_batch(logits, table, I, O, max_total, zid, allow_skip, test_mode):
    """H (B,) = -loss - risk(cost = logits) and d H / d logits (B, Imax, D) by the DP:
    d(-loss) = grad_cost (the class posterior); d risk = grad_logits + grad_cost."""
    r = expected_cost_batch(logits, logits, table, I, O, max_total, zid, allow_skip, test_mode)
    with np.errstate(invalid="ignore"):
        h = np.where(r["feasible"], -r["loss"] - r["risk"], -np.inf)
    return h, -r["grad_logits"]
