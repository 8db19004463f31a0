"""Reference of the best path on a band of the emit/shift lattice, pure numpy:
the recurrence in band coordinates, IEEE float32 adds and one strict compare per cell in the
order of DESIGN.md 2.2, written without the embedding of tests/band_ref.py; a brute force over the
paths inside the band; and the generators the CPU and GPU tests share. Test infrastructure only."""
import itertools

import numpy as np

import band_ref as BR

F32 = np.float32
NINF = F32(-np.inf)
WIDTHS = (1, 2, 3, 5, 63, 64, 65, 128, 130, 256)
T0 = 48


def dp_one(lt, lo, bs, S, P, terminal=True):
    """One utterance: lt (T,R,2) f32, lo (T,R) or None, bs (T,) of a valid band, 1 <= P <= S <= T.
    Returns (log_prob f32, position (S,) absolute or None when log_prob is -inf)."""
    lt = np.asarray(lt, F32)
    T, R, _ = lt.shape
    bs = np.asarray(bs, np.int64)
    V = np.full(R, NINF, F32)
    V[0] = lo[0, 0] if lo is not None else F32(0)
    bp = np.zeros((S, R), bool)
    with np.errstate(invalid="ignore"):
        for s in range(1, S):
            d = int(bs[s] - bs[s - 1])
            st = V + lt[s - 1, :, 0]            # V[s-1][c] + e[s-1][c], in the columns of step s-1
            mv = V + lt[s - 1, :, 1]
            stay = np.full(R, NINF, F32)        # column r of step s takes c = r + d ...
            move = np.full(R, NINF, F32)        # ... and c = r + d - 1
            if d == 0:
                stay[:] = st
                move[1:] = mv[:-1]
            else:
                stay[:-1] = st[1:]
                move[:] = mv
            bp[s] = move > stay                 # strict: a tie keeps the emit
            V = np.where(bp[s], move, stay).astype(F32)
            if lo is not None:
                V = (V + lo[s]).astype(F32)
        v = V[P - 1 - bs[S - 1]]
        if terminal:
            v = F32(v + lt[S - 1, P - 1 - bs[S - 1], 0])
    if not v > NINF:
        return NINF, None
    pos = np.zeros(S, np.int64)
    p = P - 1
    for s in range(S - 1, -1, -1):
        pos[s] = p
        if s > 0 and bp[s, p - bs[s]]:
            p -= 1
    assert p == 0
    return F32(v), pos


def dp(lt, lo, bs, S, P, terminal=True, max_pos=None):
    """The batch: lt (B,T,R,2), lo (B,T,R) or None, bs (B,T), S / P (B,). Infeasible utterances
    (S < P, S = 0, P = 0, S > T, a negative length, an invalid band, P > max_pos, log_prob -inf)
    get -inf, -1 and 0. Returns dict(log_prob (B,), position (B,T) i32, duration (B,max_pos) i32;
    max_pos defaults to max(P, 1))."""
    lt = np.asarray(lt, F32)
    B, T, R, _ = lt.shape
    U = int(max(1, np.max(P))) if max_pos is None else int(max_pos)
    out = {"log_prob": np.full(B, NINF, F32), "position": np.full((B, T), -1, np.int32),
           "duration": np.zeros((B, U), np.int32)}
    for b in range(B):
        s_, p_ = int(S[b]), int(P[b])
        if not (1 <= p_ <= s_ <= T) or p_ > U or not BR.is_valid(bs[b], s_, p_, R):
            continue
        v, pos = dp_one(lt[b], None if lo is None else lo[b], bs[b], s_, p_, terminal)
        if pos is None:
            continue
        out["log_prob"][b] = v
        out["position"][b, :s_] = pos
        out["duration"][b, :p_] = np.bincount(pos, minlength=p_)
    return out


def brute_force(lt, lo, bs, S, P, terminal=True):
    """One tiny utterance: the maximum, over every monotone path 0 -> P-1 whose cells all lie in
    the band, of the path's sequential float32 sum. Returns (log_prob, list of maximal paths)."""
    lt = np.asarray(lt, F32)
    R = lt.shape[1]
    best, arg = NINF, []
    with np.errstate(invalid="ignore"):
        for moves in itertools.combinations(range(1, S), P - 1):
            mvs = set(moves)
            v = lo[0, 0] if lo is not None else F32(0)
            p, path, ok = 0, [0], True
            for s in range(1, S):
                k = 1 if s in mvs else 0
                v = F32(v + lt[s - 1, p - bs[s - 1], k])
                p += k
                r = p - int(bs[s])
                if not 0 <= r < R:
                    ok = False
                    break
                if lo is not None:
                    v = F32(v + lo[s, r])
                path.append(p)
            if not ok:
                continue
            if terminal:
                v = F32(v + lt[S - 1, P - 1 - bs[S - 1], 0])
            if v > best:
                best, arg = v, [tuple(path)]
            elif v == best and v > NINF:
                arg.append(tuple(path))
    return best, arg


def all_valid_bands(T, S, P, R):
    """Every valid band (T,) of one (S, P, R)."""
    lo, hi = BR.end_range(S, P, R)
    out = []
    for e in range(lo, hi + 1):
        for moves in itertools.combinations(range(S - 1), e):
            out.append(BR.band_from_moves(T, S, moves))
    return out


# ---- the families of the banded forward-backward's GPU test, rebuilt here ----------------------
def utterances(R):
    """(S, P, kind, at) of the batch every width runs at T = 48."""
    M = 20  # of S = 41
    P1 = min(R + 1, 30)
    return [(48, min(R, 40), "stay", None), (48, 48, "diag", None), (45, 45, "diag", None),
            (33, 33, "diag", None), (25, 25, "diag", None), (47, 30, "alt", None),
            (45, 20, "random", None), (38, 37, "random", None), (41, P1, "at", M - 1),
            (41, P1, "at", M), (41, P1, "at", M + 1), (1, 1, "stay", None),
            (30, max(1, min(R // 2, 30)), "stay", None), (48, min(R + 7, 48), "random", None)]


def bands(R):
    """(S (B,), P (B,), band_start (B,T0)) of width R's batch; families without a band drop out."""
    rng = np.random.default_rng(R)
    rows = []
    for S, P, kind, at in utterances(R):
        bs = BR.make_band(kind, T0, S, P, R, rng, at)
        if bs is not None:
            assert BR.is_valid(bs, S, P, R)
            rows.append((S, P, bs))
    return (np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows], np.int32),
            np.stack([r[2] for r in rows]))


def synth(B, T, R, obs, seed):
    """Random log-probability pairs (log_softmax of normal logits) and a wide-range log_obs."""
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((B, T, R, 2)) * 3).astype(np.float64)
    lt = (z - np.logaddexp(z[..., :1], z[..., 1:])).astype(F32)
    lo = (rng.standard_normal((B, T, R)) * 15 - 40).astype(F32) if obs else None
    return lt, lo


def case(R, obs, seed=0):
    S, P, bs = bands(R)
    lt, lo = synth(len(S), T0, R, obs, seed + R)
    return {"lt": lt, "lo": lo, "bs": bs, "S": S, "P": P}


TIE_NINF_SHARE = 0.01


def tie_case(R, obs, seed=0):
    """The families with small-integer inputs in {0, -1, -2} and a share of -inf: most compares
    are ties or near-ties."""
    S, P, bs = bands(R)
    B = len(S)
    rng = np.random.default_rng(1000 + seed + R)
    lt = -rng.integers(0, 3, size=(B, T0, R, 2)).astype(F32)
    lt[rng.random(lt.shape) < TIE_NINF_SHARE] = NINF
    lo = None
    if obs:
        lo = -rng.integers(0, 3, size=(B, T0, R)).astype(F32)
    return {"lt": lt, "lo": lo, "bs": bs, "S": S, "P": P}
