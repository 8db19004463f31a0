"""References of the banded forward-backward, pure numpy: the embedding of a band
into a dense lattice (on which oracle.fwd_bwd_xf defines the banded result bit for bit) and the
gather back, a generator of valid bands, an independent float64 DP in band coordinates, a brute
force over the paths inside the band, and the two-block restatement of Z at the cut. Test
infrastructure only."""
import itertools

import numpy as np

F32 = np.float32
NEG = F32(-np.inf)
XF_EZERO = -(1 << 29)
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1


# ---- bands -----------------------------------------------------------------------------------
def band_from_moves(T, S, moves):
    """band_start (T,) i32 of a band that moves at the transitions in `moves` (s -> s+1, s in
    [0, S-2]); the value of step S-1 repeated beyond it."""
    bs = np.zeros(T, np.int32)
    mv = np.zeros(max(T, 1), np.int32)
    for s in moves:
        assert 0 <= s < S - 1
        mv[s] = 1
    for s in range(1, T):
        bs[s] = bs[s - 1] + (mv[s - 1] if s < S else 0)
    return bs


def end_range(S, P, R):
    """The values band_start[S-1] may take: it holds P-1 and is reachable in S-1 moves."""
    return max(0, P - R), min(P - 1, S - 1)


def make_band(kind, T, S, P, R, rng=None, at=None):
    """A valid band (T,) i32 for a feasible utterance (1 <= P <= S <= T), or None where the family
    has none at this shape. stay: never moves (P <= R); diag: moves at every step from the first
    until the last window; alt: at every other step; random: a random end and random steps; at:
    one move, at transition `at` (P <= R + 1)."""
    lo, hi = end_range(S, P, R)
    if kind == "stay":
        return band_from_moves(T, S, []) if lo == 0 else None
    if kind == "diag":
        return band_from_moves(T, S, range(hi))
    if kind == "alt":
        e = min(hi, max(lo, (S - 1) // 2))
        moves = list(range(0, S - 1, 2))[:e]
        moves += [s for s in range(1, S - 1, 2)][:e - len(moves)]
        return band_from_moves(T, S, moves)
    if kind == "random":
        e = int(rng.integers(lo, hi + 1))
        return band_from_moves(T, S, rng.choice(S - 1, size=e, replace=False) if e else [])
    assert kind == "at"
    if not (lo <= 1 <= hi and 0 <= at < S - 1):
        return None
    return band_from_moves(T, S, [at])


def is_valid(bs, S, P, R):
    bs = np.asarray(bs, np.int64)
    if S < 1 or bs[0] != 0:
        return False
    d = np.diff(bs[:S])
    return bool(np.all((d == 0) | (d == 1)) and bs[S - 1] <= P - 1 < bs[S - 1] + R)


# ---- embedding and gather -----------------------------------------------------------------------
def dense_width(bs, S, P, R):
    """U' of a batch's embedding: every band column of the steps < S_b and every position < P_b."""
    B, T = bs.shape
    w = 1
    for b in range(B):
        s = int(np.clip(S[b], 0, T))
        w = max(w, int(P[b]) if 0 < P[b] < (1 << 20) else 1)
        if s > 0:
            w = max(w, int(bs[b, :s].max()) + R)
    return w


def embed(lt_band, lo_band, bs, S, P, U=None):
    """The dense lattice (log_trans (B,T,U',2), log_obs (B,T,U') or None) that is the band inside
    it, -inf (log_obs 0) outside it, and -inf on the edges that leave it: the shift out of r = R-1
    where the band stays, the emit out of r = 0 where it moves. Bands must be valid at s < S_b."""
    lt_band = np.asarray(lt_band, F32)
    B, T, R, _ = lt_band.shape
    bs = np.asarray(bs, np.int64)
    U = dense_width(bs, S, P, R) if U is None else U
    lt = np.full((B, T, U, 2), NEG, F32)
    lo = None if lo_band is None else np.zeros((B, T, U), F32)
    for b in range(B):
        for s in range(int(np.clip(S[b], 0, T))):
            p0 = int(bs[b, s])
            row = np.array(lt_band[b, s], F32)
            if s + 1 < S[b]:
                if bs[b, s + 1] == p0:
                    row[R - 1, 1] = NEG
                else:
                    row[0, 0] = NEG
            n = min(R, U - p0)
            lt[b, s, p0:p0 + n] = row[:n]
            if lo is not None:
                lo[b, s, p0:p0 + n] = lo_band[b, s, :n]
    return lt, lo


def gather(dense, bs, R, S=None, fill=0):
    """dense (B,T,U,...) -> (B,T,R,...): out[b,s,r] = dense[b,s,bs[b,s]+r], `fill` outside [0, U)
    and, with S, at steps >= S_b."""
    dense = np.asarray(dense)
    B, T, U = dense.shape[:3]
    idx = np.asarray(bs, np.int64)[:, :, None] + np.arange(R)
    ok = (idx >= 0) & (idx < U)
    if S is not None:
        ok &= (np.arange(T)[None, :] < np.asarray(S).reshape(B, 1))[:, :, None]
    shape = idx.shape + (1,) * (dense.ndim - 3)
    out = np.take_along_axis(dense, np.clip(idx, 0, U - 1).reshape(shape), axis=2)
    out[~ok] = fill
    return out


def dead_mask(bs, S, P, R, terminal):
    """(mask_trans (B,T,R,2), mask_obs (B,T,R)) bool: the band cells the contract never reads:
    rows s >= S_b; columns at p >= P_b; the shift out of p = P_b - 1; every entry of row S_b - 1
    but the terminal emit (that one too without it); the shift out of r = R-1 where the band stays
    and the emit out of r = 0 where it moves. Valid bands, feasible lengths."""
    B, T = bs.shape
    mt = np.zeros((B, T, R, 2), bool)
    mo = np.zeros((B, T, R), bool)
    for b in range(B):
        s_, p_ = int(S[b]), int(P[b])
        mt[b, s_:] = True
        mo[b, s_:] = True
        for s in range(s_):
            p = int(bs[b, s]) + np.arange(R)
            mt[b, s, p >= p_] = True
            mo[b, s, p >= p_] = True
            mt[b, s, p == p_ - 1, 1] = True
            if s == s_ - 1:
                mt[b, s] = True
                if terminal:
                    mt[b, s, p == p_ - 1, 0] = False
            elif bs[b, s + 1] == bs[b, s]:
                mt[b, s, R - 1, 1] = True
            else:
                mt[b, s, 0, 0] = True
    return mt, mo


def oracle_band(O, lt_band, lo_band, bs, S, P, flags=1):
    """The banded result by its definition: oracle.fwd_bwd_xf on the embedding, gathered. Also
    returns the dense gradients ("dense_grad", "dense_grad_obs") and the embedding's width."""
    R = np.asarray(lt_band).shape[2]
    lt, lo = embed(lt_band, lo_band, bs, S, P)
    U = lt.shape[2]
    # (lengths the banded call judges without a U: P_b > U' cannot occur for a valid band)
    o = O.fwd_bwd_xf(lt, np.asarray(S, np.int32), np.asarray(P, np.int32), lo, flags=flags)
    out = {"loss": o["loss"], "grad": gather(o["grad"], bs, R, S), "dense_grad": o["grad"], "U": U}
    if lo is not None:
        out["grad_obs"] = gather(o["grad_obs"], bs, R, S)
        out["dense_grad_obs"] = o["grad_obs"]
    return out


# ---- float64 DP in band coordinates (one utterance) -------------------------------------------
def band_dp64(lt, lo, bs, S, P, terminal=True):
    """Independent float64 log-domain DP over band cells: lt (T,R,2), lo (T,R) or None, bs (T,).
    Returns loss, grad (T,R,2), grad_obs (T,R) (None without lo). Inputs finite or -inf."""
    lt = np.asarray(lt, np.float64)
    T, R, _ = lt.shape
    ob = np.zeros((T, R)) if lo is None else np.asarray(lo, np.float64)
    bs = np.asarray(bs, np.int64)
    la = np.full((S, R), -np.inf)
    lb = np.full((S, R), -np.inf)
    live = lambda s, r: 0 <= r < R and bs[s] + r < P  # noqa: E731

    def edges(s, r):  # (k, r') of the edges out of (s, r) that stay inside the band and the lattice
        d = int(bs[s + 1] - bs[s])
        out = []
        if live(s + 1, r - d):
            out.append((0, r - d))
        if bs[s] + r < P - 1 and live(s + 1, r + 1 - d):
            out.append((1, r + 1 - d))
        return out

    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        la[0, 0] = ob[0, 0]
        for s in range(S - 1):
            for r in range(R):
                if live(s, r) and la[s, r] > -np.inf:
                    for k, r2 in edges(s, r):
                        la[s + 1, r2] = np.logaddexp(la[s + 1, r2], la[s, r] + lt[s, r, k] + ob[s + 1, r2])
        rl = P - 1 - int(bs[S - 1])
        lb[S - 1, rl] = lt[S - 1, rl, 0] if terminal else 0.0
        for s in range(S - 2, -1, -1):
            for r in range(R):
                if live(s, r):
                    for k, r2 in edges(s, r):
                        lb[s, r] = np.logaddexp(lb[s, r], lt[s, r, k] + ob[s + 1, r2] + lb[s + 1, r2])
        logz = la[S - 1, rl] + lb[S - 1, rl]
        grad = np.zeros((T, R, 2))
        gobs = np.zeros((T, R))
        if logz == -np.inf:
            return np.inf, grad, (None if lo is None else gobs)
        for s in range(S):
            for r in range(R):
                if not live(s, r) or la[s, r] == -np.inf:
                    continue
                if lb[s, r] > -np.inf:
                    gobs[s, r] = -np.exp(la[s, r] + lb[s, r] - logz)
                if s == S - 1:
                    if terminal and r == rl:
                        grad[s, r, 0] = -1.0
                    continue
                for k, r2 in edges(s, r):
                    v = la[s, r] + lt[s, r, k] + ob[s + 1, r2] + lb[s + 1, r2] - logz
                    if v > -np.inf:
                        grad[s, r, k] = -np.exp(v)
    return -logz, grad, (None if lo is None else gobs)


# ---- brute force over the paths inside the band (one utterance, tiny) --------------------------
def brute_force(lt, lo, bs, S, P, terminal=True):
    """Every monotone path 0 -> P-1 over S steps whose cells all lie in the band, summed in
    float64. Returns loss, grad (T,R,2), grad_obs (T,R)."""
    lt = np.asarray(lt, np.float64)
    T, R, _ = lt.shape
    ob = np.zeros((T, R)) if lo is None else np.asarray(lo, np.float64)
    paths = []
    for ks in itertools.product((0, 1), repeat=S - 1):
        if sum(ks) != P - 1:
            continue
        p, w, ok = 0, ob[0, 0], True
        cells = [(0, 0)]
        for s, k in enumerate(ks):
            w += lt[s, p - bs[s], k]
            p += k
            r = p - int(bs[s + 1])
            if not 0 <= r < R:
                ok = False
                break
            w += ob[s + 1, r]
            cells.append((s + 1, r))
        if ok:
            if terminal:
                w += lt[S - 1, p - bs[S - 1], 0]
            paths.append((w, ks, cells))
    grad = np.zeros((T, R, 2))
    gobs = np.zeros((T, R))
    ws = np.array([w for w, _, _ in paths])
    if len(ws) == 0 or np.all(ws == -np.inf):
        return np.inf, grad, gobs
    logz = np.logaddexp.reduce(ws)
    for w, ks, cells in paths:
        q = np.exp(w - logz)
        for (s, r), k in zip(cells, ks):
            grad[s, r, k] -= q
        if terminal:
            grad[cells[-1][0], cells[-1][1], 0] -= q
        for s, r in cells:
            gobs[s, r] -= q
    return -logz, grad, gobs


# ---- the two-block restatement of Z at the cut ------------------------------------------------
def xf_add(a, b):
    """xf_math.h xf_add on (m f32, e int) pairs."""
    (ma, ea), (mb, eb) = a, b
    em = max(ea, eb)
    with np.errstate(under="ignore"):
        s = F32(np.ldexp(F32(ma), max(ea - em, -400))) + F32(np.ldexp(F32(mb), max(eb - em, -400)))
    if s == 0:
        return F32(0), XF_EZERO
    m, k = np.frexp(F32(s))
    return F32(m), em + int(k)


def tree(w):
    """Binary tree, pairs (2i, 2i+1) first, over a power-of-two list of xf pairs."""
    w = list(w)
    while len(w) > 1:
        w = [xf_add(w[2 * i], w[2 * i + 1]) for i in range(len(w) // 2)]
    return w[0]


def two_block_z(alpha, beta, bs, S, P, R):
    """Z of one utterance from the dense state rows alpha / beta (T,U) of oracle.XF_DTYPE at the
    cut row M, the way the banded kernel forms it: products at p - base in 2R' zero slots, one tree
    per aligned block, one add."""
    M = (S - 1) >> 1
    Rp = 1
    while Rp < R:
        Rp <<= 1
    base = (int(bs[M]) // Rp) * Rp
    slots = [(F32(0), XF_EZERO)] * (2 * Rp)
    for r in range(R):
        p = int(bs[M]) + r
        if p < P:
            a, b = alpha[M, p], beta[M, p]
            slots[p - base] = (F32(a["m"]) * F32(b["m"]), int(a["e"]) + int(b["e"]))
    return xf_add(tree(slots[:Rp]), tree(slots[Rp:]))
