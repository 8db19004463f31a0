"""Float64 reference for posterior sampling on the v2 duration-class lattice.

``forward``: the alpha recurrence of one utterance as a numpy log-domain DP over F4's windows
(`v2_viterbi_ref.window`). ``draw``: the backward walk, vectorised over the samples: the final total
from the exact CDF of row I, then for r = I..1 the class from the exact CDF `cum/total` of the D
terms entering the cell -- the lowest class with a positive term and u < cum_i/total, else the
highest with a positive term. Each sample also gets its margin, min |u - c| over every interior
boundary (0 < c < 1) of every categorical it visited, the final total's included: a sample whose
margin exceeds DELTA is *clear*, and an f32 implementation must reproduce its classes and total
exactly (a forced choice has no interior boundary and is exact on both sides).
``path_log_prob_f32`` restates the sequential f32 sum of a sequence; ``path_posterior`` enumerates
every admissible sequence of a tiny utterance through `f4_cases.move_ok`; ``clear_uniforms`` makes
uniforms under which (almost) every sample is clear. Test infrastructure only."""
import functools

import numpy as np

import v2_viterbi_ref as VR
from f4_cases import move_ok, random_case

F32 = np.float32
DELTA = 1e-4
U_MAX = F32(1.0) - F32(2.0 ** -24)
LOG_MIN = -1.0e6  # log-probs below this are exact zeros (xf_exp)


def clamp_uniform(u):
    """The kernel's clamp, in f32: NaN -> 0, then [0, 1 - 2^-24]."""
    u = np.asarray(u, F32)
    u = np.where(u >= 0, u, F32(0))
    return np.minimum(u, U_MAX).astype(F32)


def _weights(logits, zid, allow_skip):
    w = np.asarray(logits, np.float64).copy()
    w[~(w >= LOG_MIN)] = -np.inf
    if not allow_skip:
        w[:, zid] = -np.inf
    return w


def forward(logits, table, I, O, max_total, zid, allow_skip, test_mode):
    """One utterance (logits (T,D)): None when it has no lattice or Z = 0, else the dict draw()
    walks: la (I+1, X) log alpha in float64 (-inf outside the windows), w (T,D), table."""
    logits = np.asarray(logits, F32)
    table = np.asarray(table, np.int64)
    T, D = logits.shape
    X = int(max_total) + 1
    I, O = int(I), int(O)
    if (table < 0).any() or I < 1 or I > T or O < 0 or (not test_mode and O > X - 1):
        return None
    dmax = int(table.max())
    w = _weights(logits, zid, allow_skip)
    la = np.full((I + 1, X), -np.inf)
    la[0, 0] = 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        for r in range(1, I + 1):
            lo, hi = VR.window(r, I, O, X, dmax, test_mode)
            if hi < lo:
                return None
            terms = np.full((D, hi - lo + 1), -np.inf)
            for i in range(D):
                d = int(table[i])
                a, b = max(lo - d, 0), hi - d  # source cells [a, b] -> cells [a + d, hi]
                if b >= a and w[r - 1, i] > -np.inf:
                    terms[i, a + d - lo:] = la[r - 1, a:b + 1] + w[r - 1, i]
            m = terms.max(0)
            live = m > -np.inf
            row = np.full(hi - lo + 1, -np.inf)
            row[live] = m[live] + np.log(np.exp(terms[:, live] - m[live]).sum(0))
            la[r, lo:hi + 1] = row
    if not (la[I] > -np.inf).any():
        return None
    return {"la": la, "w": w, "table": table, "I": I, "T": T, "X": X}


def _choose(t, u):
    """t (K,N) log terms, u (K,) f32 -> (choice (K,), margin (K,)): the rule of DESIGN.md 2.5 with
    the exact CDF."""
    K, N = t.shape
    m = t.max(1, keepdims=True)
    assert np.all(m > -np.inf)
    p = np.exp(t - m)
    cum = np.cumsum(p, 1)
    cdf = cum / cum[:, -1:]
    uu = u.astype(np.float64)[:, None]
    pos = p > 0
    hit = pos & (uu < cdf)
    first = np.where(hit.any(1), hit.argmax(1), N - 1 - pos[:, ::-1].argmax(1))
    inner = (cdf > 0) & (cdf < 1)
    gap = np.where(inner, np.abs(uu - cdf), np.inf)
    return first, gap.min(1)


def draw(fw, u):
    """fw from forward(), u (K,T+1) -> duration_class (K,T), duration (K,T), total (K,), margin (K,)."""
    u = clamp_uniform(u)
    K = u.shape[0]
    la, w, table, I, T, X = (fw[k] for k in ("la", "w", "table", "I", "T", "X"))
    cls_out = np.full((K, T), -1, np.int32)
    dur_out = np.zeros((K, T), np.int32)
    x, margin = _choose(np.broadcast_to(la[I], (K, X)), u[:, T])
    total = x.astype(np.int32)
    ar = np.arange(K)
    with np.errstate(invalid="ignore"):
        for r in range(I, 0, -1):
            y = x[:, None] - table[None, :]
            t = np.where(y >= 0, la[r - 1][np.clip(y, 0, X - 1)], -np.inf) + w[r - 1][None, :]
            c, g = _choose(t, u[:, r - 1])
            margin = np.minimum(margin, g)
            cls_out[:, r - 1] = c
            dur_out[:, r - 1] = table[c]
            x = y[ar, c]
    assert np.all(x == 0)
    return {"duration_class": cls_out, "duration": dur_out, "total": total, "margin": margin}


def _empty(K, T):
    return {"duration_class": np.full((K, T), -1, np.int32), "duration": np.zeros((K, T), np.int32),
            "total": np.full(K, -1, np.int32), "margin": np.full(K, np.inf)}


def sample_batch(case, u, fws=None):
    """case = (logits (B,T,D), table, I, O, max_total, allow_skip, test_mode) (zero_duration_id 0),
    u (B,K,T+1): feasible (B,), duration_class (B,K,T), duration, total (B,K), margin (B,K)."""
    logits = case[0]
    B, T, _ = logits.shape
    K = u.shape[1]
    fws = forwards(case) if fws is None else fws
    rs = [draw(fw, u[b]) if fw is not None else _empty(K, T) for b, fw in enumerate(fws)]
    res = {k: np.stack([r[k] for r in rs]) for k in rs[0]}
    res["feasible"] = np.array([fw is not None for fw in fws])
    return res


def forwards(case):
    logits, table, I, O, mt, allow_skip, test_mode = case
    return [forward(logits[b], table, I[b], O[b], mt, 0, allow_skip, test_mode) for b in range(len(I))]


def clear(res):
    """(B,K) bool: the samples an f32 implementation must reproduce exactly."""
    return (res["margin"] > DELTA) & res["feasible"][:, None]


def clear_uniforms(case, K, seed, rounds=16):
    """Uniforms (B,K,T+1) f32 for `case` and the reference's result under them: i.i.d. to begin
    with, then the row of every sample whose margin is not above DELTA is drawn again, at most
    `rounds` times, from a generator seeded by (seed, round) -- deterministic."""
    logits = case[0]
    B, T, _ = logits.shape
    fws = forwards(case)
    u = np.random.default_rng([seed, 0]).random((B, K, T + 1), dtype=F32)
    res = sample_batch(case, u, fws)
    for rnd in range(1, rounds + 1):
        bad = ~(res["margin"] > DELTA) & res["feasible"][:, None]
        if not bad.any():
            break
        fresh = np.random.default_rng([seed, rnd]).random((B, K, T + 1), dtype=F32)
        for b in np.flatnonzero(bad.any(1)):
            ks = np.flatnonzero(bad[b])
            u[b, ks] = fresh[b, ks]
            r = draw(fws[b], u[b, ks])
            for key, v in r.items():
                res[key][b, ks] = v
    return u, res


def path_log_prob_f32(logits, classes):
    """The sequential f32 sum of DESIGN.md 2.5: logits (T,D), classes (T,) with -1 beyond I."""
    logits = np.asarray(logits, F32)
    v = F32(0)
    with np.errstate(invalid="ignore"):
        for t, c in enumerate(np.asarray(classes)):
            if c < 0:
                break
            v = F32(v + logits[t, c])
    return v


def path_posterior(logits, table, I, O, max_total, zid, allow_skip, test_mode):
    """Every admissible class sequence of one tiny utterance (depth first, cut at the first move
    f4_cases.move_ok refuses) with its posterior probability in float64:
    {(classes..., total): probability}; {} when there is none."""
    logits = np.asarray(logits, np.float64)
    D = logits.shape[1]
    X = max_total + 1
    assert I <= 8
    seqs, scores = [], []

    def walk(t, tot, sc, seq):
        if t == I:
            seqs.append(tuple(seq) + (tot,))
            scores.append(sc)
            return
        for i in range(D):
            nt = tot + int(table[i])
            if not move_ok(t, nt, i, I, O, X, zid, allow_skip, test_mode) or not logits[t, i] >= LOG_MIN:
                continue
            walk(t + 1, nt, sc + logits[t, i], seq + [i])

    if I >= 1:
        walk(0, 0, 0.0, [])
    if not seqs:
        return {}
    scores = np.array(scores)
    wgt = np.exp(scores - scores.max())
    return dict(zip(seqs, wgt / wgt.sum()))


def frequency_deviation(classes, totals, I, post, floor=1e-3):
    """classes (N,T), totals (N,) drawn for one utterance; post from path_posterior. The largest
    |frequency - posterior| in binomial standard deviations over the sequences with posterior >=
    floor; every drawn sequence must be one of the lattice's."""
    N = classes.shape[0]
    keys, counts = np.unique(np.concatenate([classes[:, :I], totals[:, None]], 1), axis=0, return_counts=True)
    seen = {tuple(int(x) for x in k): int(c) for k, c in zip(keys, counts)}
    assert set(seen) <= set(post), "a drawn sequence is not a path of the lattice"
    worst = 0.0
    for path, q in post.items():
        if q < floor:
            continue
        if q == 1.0:
            assert seen.get(path, 0) == N
            continue
        worst = max(worst, abs(seen.get(path, 0) / N - q) / np.sqrt(q * (1 - q) / N))
    return worst


# ---- the case families the GPU file holds to the reference sample by sample -------------------
def _random_family(seed, Imax, D, table, mode, B=6, slack=5):
    """f4_cases.random_case with durations near O/I; band mode needs O >= 3 (I - 1)."""
    rng = np.random.default_rng(seed)
    logits, I, _ = random_case(rng, B, Imax, D)
    table = np.asarray(table, np.int32)
    dmax = int(table.max())
    lo = 3 if dmax >= 6 else 1
    O = np.array([int(rng.integers(lo * i, max(lo * i, (dmax * i) // 2) + 1)) for i in I], np.int32)
    test_mode, allow_skip = mode == "test_mode", mode != "no_skip"
    return logits, table, I, O, int(O.max()) + (slack if test_mode else 0), allow_skip, test_mode


def tables_case(name, test_mode):
    """The duration tables of test_gpu_v2_viterbi.py at its shape (B=5, I = 150/149/97/70/20): class
    slots 8/16/32/64, the padded and the clamped cell form, dmax > 63. O sums I random durations,
    so a path inside the band exists."""
    from test_gpu_v2_viterbi import F4_TABLES, _softmax_logits
    table = np.array(dict(F4_TABLES)[name], np.int32)
    D = len(table)
    B, Imax = 5, 150
    rng = np.random.default_rng(D)
    logits = _softmax_logits(rng, (B, Imax, D))
    I = np.array([150, 149, 97, 70, 20], np.int32)
    O = np.array([int(table[rng.integers(0, D, size=i)].sum()) for i in I], np.int32)
    return logits, table, I, O, int(O.max()) + (7 if test_mode else 0), True, bool(test_mode)


TABLE_NAMES = ["long_durations", "shuffled16", "d20", "d40"]

# name -> (K, builder): every family the GPU file draws with clear_uniforms
FAMILIES = {}
for _seed in range(6):
    for _mode in VR.MODES:
        FAMILIES[f"tiny-{_seed}-{_mode}"] = (16, functools.partial(VR.tiny_case, _seed, _mode))
for _mode in ("band", "test_mode"):
    # dmax 21: two steps per round trip; dmax 15: four; D = 64, dmax 63: one gather per step
    FAMILIES[f"i24d8-{_mode}"] = (8, functools.partial(_random_family, 24, 24, 8, [0, 1, 2, 3, 5, 8, 13, 21], _mode))
    FAMILIES[f"i40d16-{_mode}"] = (8, functools.partial(_random_family, 40, 40, 16, np.arange(16), _mode))
    for _name in TABLE_NAMES:
        FAMILIES[f"table-{_name}-{_mode}"] = (4, functools.partial(tables_case, _name, _mode == "test_mode"))
FAMILIES["i12d64-test_mode"] = (8, functools.partial(_random_family, 12, 12, 64, np.arange(64), "test_mode"))


def value_case(name, test_mode, B=4, Imax=32, D=8):
    """One input value class of tests/value_cases.py on teacher-forced logits (B=4, I=32 ragged,
    D=8, durations 0..7, O the planted durations' sum, so a path inside the band exists)."""
    import oracle as O
    import value_cases as VC
    d = O.synth_durations(B, Imax, 4 * Imax, D, seed=32)
    logits = VC.v2(name, O.synth_v2_step_logits(d, D, seed=33))
    I = np.array([Imax, Imax - 5, Imax - 2, Imax - 11], np.int32)
    Ol = np.array([int(d[b, :I[b]].sum()) for b in range(B)], np.int32)
    return logits, np.arange(D, dtype=np.int32), I, Ol, int(Ol.max()) + (20 if test_mode else 0), True, bool(test_mode)


VALUE_CLASSES = ("peaked30", "saturated_emit", "plus88", "minus1e4", "alt_rows", "alt_cols")  # = VC.TOLERANCE_CLASSES
for _name in VALUE_CLASSES:
    for _mode in ("band", "test_mode"):
        FAMILIES[f"value-{_name}-{_mode}"] = (16, functools.partial(value_case, _name, _mode == "test_mode"))


@functools.lru_cache(maxsize=None)
def family(name, seed=0):
    """(case, K, u, reference result) of one family, computed once."""
    K, build = FAMILIES[name]
    case = build()
    u, res = clear_uniforms(case, K, seed)
    return case, K, u, res
