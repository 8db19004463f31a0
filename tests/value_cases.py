"""Named input value classes of the lattice tests (DESIGN.md 3 "Input domain"): what a caller can
bring beyond log_softmax of tame logits -- saturated softmaxes, unnormalised positive scores, frame
log-likelihoods in the hundreds, exponents of 1e4 .. 1e6 per step, neighbouring terms 2^230 apart,
the live / dead boundary of xf_exp and NaN in live cells. One table per input kind: every class is a
function (base array, rng) -> f32 array of the same shape, where base is oracle.synth_log_trans
(B,T,U,2) or oracle.synth_v2_step_logits (B,I,D). Pure numpy; the CPU references are held to the
conditions the GPU tests rely on in tests/test_value_cases_ref.py, the GPU tests are
tests/test_gpu_value_ranges.py. Test infrastructure only."""
import numpy as np

F32 = np.float32
LOG_MIN, LOG_MAX = F32(-1.0e6), F32(1.0e6)  # XF_LOG_MIN / XF_LOG_MAX of xf_math.h
# the cells of `threshold`, in turn: the last live value, the first dead one, -inf, the clamp
# value, and two values above it
THRESHOLD_VALUES = np.array([LOG_MIN, np.nextafter(LOG_MIN, F32(-np.inf)), -np.inf, LOG_MAX, 1e30, np.inf], F32)


def _log_softmax(z):
    m = z.max(axis=-1, keepdims=True)
    return (z - (m + np.log(np.exp(z - m).sum(axis=-1, keepdims=True)))).astype(F32)


def _peaked(scale):
    """oracle.synth_log_trans(scale=scale): values to -5 * scale, so most factors of `peaked30`
    are subnormal or zero as an f32, beside factors near 1"""
    return lambda base, rng: _log_softmax(rng.standard_normal(base.shape, dtype=F32) * F32(scale))


def _const(*values):
    def f(base, rng):
        out = np.empty_like(base, dtype=F32)
        out[...] = np.asarray(values, F32)
        return out
    return f


def _shift(delta):
    return lambda base, rng: (base + F32(delta)).astype(F32)


def _alternating(axis, delta=80.0):
    def f(base, rng):
        shape = [1] * base.ndim
        shape[axis] = base.shape[axis]
        sign = np.where(np.arange(base.shape[axis]) % 2 == 0, F32(delta), F32(-delta)).reshape(shape)
        return (base + sign).astype(F32)
    return f


def _scatter(base, rng, values, share=0.1):
    """`share` of the cells, each set to one of `values` in turn (by bit pattern)."""
    out = np.array(base, F32)
    idx = np.flatnonzero(rng.random(base.size) < share)
    out.reshape(-1)[idx] = np.asarray(values, F32)[np.arange(idx.size) % len(values)]
    return out


def _threshold(base, rng):
    return _scatter(base, rng, THRESHOLD_VALUES)


def _nan_live(base, rng):
    return _scatter(base, rng, [np.nan])


def _patches(base, rng):
    """The four patches of test_gpu_fwd_bwd.py::test_wide_extreme_factors scaled to the shape: a
    factor that is subnormal as an f32 (-100), below every subnormal (-200, -1e4) and beyond f32
    (+100), on either side of the streaming kernel's cut M = (S-1) >> 1 and across it."""
    out = np.array(base, F32)
    B, T, U = out.shape[:3]
    W = min(T, U)  # the positions every full-length utterance has
    out[1 % B, T // 16:T // 4, W // 30:W // 4 + 1, 0] = -100.0        # first half of the steps
    out[0, (5 * T) // 8:(7 * T) // 8, W // 2:(2 * W) // 3 + 1, 1] = -200.0  # second half
    out[0, (3 * T) // 8:(5 * T) // 8, W // 4:W // 2, :] = 100.0       # across the middle
    out[B - 1, T // 8:T // 8 + 3, :, 1] = -1.0e4                     # every position of 3 steps
    return out


# name -> (base log_trans (B,T,U,2), rng) -> log_trans
LATTICE = {
    "peaked10": _peaked(10.0),
    "peaked30": _peaked(30.0),
    "saturated_emit": _const(-1e-7, -16.0),   # exp rounds to 1 - ulp; near one-path posterior
    "saturated_shift": _const(-103.0, 0.0),   # the other single-path regime (run with S == P)
    "zeros": _const(0.0),                     # alpha are binomials, doubling every step
    "mant_hi": _const(0.34),                  # factor mantissa 1.40: x2.8 per step, the fastest growth
    "mant_lo": _const(-0.34),                 # factor mantissa 0.71: the fastest shrink on one path
    "plus40": _shift(40.0),
    "plus88": _shift(88.0),                   # exp(88) at the f32 edge
    "minus1e4": _shift(-1.0e4),
    "minus9e5": _shift(-9.0e5),
    "alt_rows": _alternating(1),              # neighbouring terms 2^230 apart, both signs
    "alt_cols": _alternating(2),
    "patches": _patches,
    "threshold": _threshold,
    "nan_live": _nan_live,
    "near_envelope": _shift(-9.9e5),          # at NEAR_ENVELOPE's shape only
}
# the closest a test goes to XF_EZERO = -2^29, from the inside: cumulative log-probability
# -9.9e5 * 299 = -2.96e8, an exponent of -4.3e8
NEAR_ENVELOPE = {"shape": (2, 300, 8), "S": [300, 297], "P": [8, 5]}
# the classes every shape runs (near_envelope has its own)
LATTICE_CLASSES = [n for n in LATTICE if n != "near_envelope"]
# classes whose inputs hold NaN, values below -1e6 or above +1e6: compared through as_neg_inf /
# as_clamped where a reference does not define them
CLEANED = ("threshold", "nan_live", "obs_nan_live")

# name -> (base log_obs (B,T,U), rng) -> log_obs; each used with base and peaked30 transitions
OBS = {
    "obs_frames": lambda base, rng: (rng.standard_normal(base.shape) * 100 - 300).astype(F32),
    "obs_zero": _const(0.0),
    "obs_holes": lambda base, rng: _scatter(base, rng, [-np.inf]),
    "obs_nan_live": _nan_live,
}

# name -> (base logits (B,I,D), rng) -> logits; alt_cols alternates by class
V2 = {
    "peaked30": _peaked(30.0),
    "zeros": _const(0.0),
    "mant_hi": _const(0.34),
    "plus88": _shift(88.0),
    "minus1e4": _shift(-1.0e4),
    "minus9e5": _shift(-9.0e5),
    "alt_rows": _alternating(1),
    "alt_cols": _alternating(2),
    "threshold": _threshold,
    "nan_live": _nan_live,
}

# the classes of the exact path entries (finite or -inf inputs only) and of the tolerance-bound ones
PATH_CLASSES = ("peaked30", "saturated_emit", "zeros", "plus88", "minus9e5", "alt_rows", "alt_cols")
TOLERANCE_CLASSES = ("peaked30", "saturated_emit", "plus88", "minus1e4", "alt_rows", "alt_cols")
# saturated_emit on the v2 logits (the tolerance-bound and path entries): one class at -1e-7, the
# others at -16
V2_EXTRA = {"saturated_emit": lambda base, rng: np.where(
    np.arange(base.shape[-1]) == np.argmax(base, axis=-1)[..., None], F32(-1e-7), F32(-16.0)).astype(F32)}


def _rng(name, seed):
    return np.random.default_rng([seed, sum(name.encode())])


def lattice(name, base, seed=0):
    return LATTICE[name](np.asarray(base, F32), _rng(name, seed))


def obs(name, shape, seed=0):
    rng = _rng(name, seed)
    base = (rng.standard_normal(shape) * 15 - 40).astype(F32)  # the suite's usual N(-40, 15^2)
    return OBS[name](base, rng)


def v2(name, base, seed=0):
    f = V2[name] if name in V2 else V2_EXTRA[name]
    return f(np.asarray(base, F32), _rng(name, seed))


def as_neg_inf(x):
    """Every NaN and every value below -1e6 replaced by -inf: what xf_exp reads them as."""
    x = np.array(x, F32)
    x[~(x >= LOG_MIN)] = -np.inf
    return x


def as_clamped(x):
    """Every value above +1e6 replaced by +1e6: what xf_exp reads them as."""
    x = np.array(x, F32)
    x[x > LOG_MAX] = LOG_MAX
    return x


def cleaned(x):
    return None if x is None else as_neg_inf(as_clamped(x))


def _same_mod4(s, limit):
    """The largest value <= limit that is s modulo 4 (at least 1)."""
    return max(s - 4 * max(0, -(-(s - limit) // 4)), 1)


def lengths(B, T, U, kind="ragged"):
    """(S, P) of a batch. The streaming chains normalise every 4th step, so S mod 4 takes as many
    of 0..3 as the batch has utterances.
    ragged: utterance 0 has every step and min(U, 3T/4) positions (many paths also where T < U);
      the last one S == P; of the others the first is ragged in both extents and the second has
      P == 1.
    diag:   S == P everywhere (one path, every move a shift).
    single: S == P and P == 1 in turn (one path each), S ragged."""
    S = [T - b - 4 * ((3 * b) % 5) for b in range(B)]
    W = min(T, U)
    if kind == "diag":
        S = [_same_mod4(s, W) for s in S]
        return np.array(S, np.int32), np.array(S, np.int32)
    if kind == "single":
        S = [_same_mod4(s, W) if b % 2 == 0 else s for b, s in enumerate(S)]
        return np.array(S, np.int32), np.array([s if b % 2 == 0 else 1 for b, s in enumerate(S)], np.int32)
    assert kind == "ragged"
    P = [min(U, T - T // 4)] + [max(1, (2 * min(U, s)) // 3) for s in S[1:]]
    if B >= 4:
        P[2] = 1
    if B >= 2:
        S[B - 1] = _same_mod4(S[B - 1], W)
        P[B - 1] = S[B - 1]
    return np.array(S, np.int32), np.array(P, np.int32)


# the lengths each class runs with ("ragged" unless named here)
LENGTH_KINDS = {"saturated_shift": ("diag",), "mant_lo": ("ragged", "single")}


def length_kinds(name):
    return LENGTH_KINDS.get(name, ("ragged",))
