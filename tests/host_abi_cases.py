"""Cases of the host-pointer C ABI tests (tests/test_gpu_host_abi.py): one call of a reference
symbol or of ssnt_fwd_bwd through ssnt_tts_amd.capi, with its reference from the C oracle.

A case is built, and its reference computed, on the thread that calls the builder (the main
thread: the oracle's thread safety is not established). `run()` then makes the call on whatever
thread calls it and returns None, or a description of the first output that differs."""
import numpy as np

import decode_cases as dc

V1_KEYS = ("prediction", "log_prob", "next_t", "next_u", "next_is_finished", "beam_branch")
V2_KEYS = ("prediction", "log_prob", "next_t", "next_u", "next_is_finished",
           "next_total_duration", "beam_branch")
FB_KEYS = ("loss", "grad", "grad_obs", "log_alpha", "log_beta")
MIB = 1 << 20


def same(a, b):
    """Equal values cell for cell (NaN equals NaN), equal shapes and types."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind == "f":
        return bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())
    return bool(np.array_equal(a, b))


class Case:
    """name; call(capi) -> the outputs, in the order of `want`; plan_bytes: the sum of the arrays
    the call stages (the library pads each to 256 B and adds a status word)."""

    def __init__(self, name, call, want, plan_bytes):
        self.name, self.call, self.want, self.plan_bytes = name, call, list(want), plan_bytes

    def run(self, capi):
        got = self.call(capi)
        if len(got) != len(self.want):
            return f"{self.name}: {len(got)} outputs, expected {len(self.want)}"
        for i, (g, w) in enumerate(zip(got, self.want)):
            if not same(g, w):
                bad = np.argwhere(np.asarray(g) != np.asarray(w))[:3].tolist() if np.shape(g) == np.shape(w) else "shape"
                return f"{self.name}: output {i} differs at {bad}"
        return None


def _nbytes(*arrays):
    return int(sum(np.asarray(a).nbytes for a in arrays))


def v1_step(oracle, seed, W=None):
    c = dc.v1_case(seed, B=1, W=W)
    W = c["h"].shape[1]
    o = oracle.v1_step(c["h"], c["hist"], c["fin"], c["t"], c["u"], c["input_length"])
    want = [o[k][0] for k in V1_KEYS]
    return Case(f"v1(seed={seed},W={W})",
                lambda capi: capi.ssnt_tts_beam_search_decode(
                    c["h"][0], c["hist"][0], c["fin"][0], c["t"][0], c["u"][0],
                    int(c["input_length"][0]), W),
                want, _nbytes(c["h"], c["hist"], c["fin"], c["t"], c["u"], *want))


def _v2(oracle, c, name):
    B, W, D = c["h"].shape
    o, rc = oracle.v2_step(c["h"], c["hist"], c["fin"], c["total"], c["table"], c["t"], c["u"],
                           c["input_length"], c["output_length"], c["zero_duration_id"],
                           c["allow_skip"], c["test_mode"])
    if rc != 0:
        return None  # no candidate: the reference symbol would abort
    want = [o[k] for k in V2_KEYS]
    return Case(name,
                lambda capi: capi.ssnt_tts_v2_beam_search_decode(
                    c["h"], c["hist"], c["fin"], c["total"], c["table"], c["t"], c["u"],
                    c["input_length"], c["output_length"], B, W, D, c["zero_duration_id"],
                    c["allow_skip"], c["test_mode"]),
                want, _nbytes(c["h"], c["hist"], c["fin"], c["total"], c["table"], c["t"], c["u"],
                              c["input_length"], c["output_length"], *want))


def v2_step(oracle, seed):
    """The first seed from `seed` on whose state has candidates (so the symbol does not abort)."""
    for s in range(seed, seed + 50):
        case = _v2(oracle, dc.v2_case(s), f"v2(seed={s})")
        if case is not None:
            return case
    raise AssertionError("no v2 case with candidates")


def v2_step_sized(oracle, seed, B, W, D):
    """Beams near the diagonal of a long utterance (decode_cases.v2_case_long): candidates exist."""
    case = _v2(oracle, dc.v2_case_long(seed, W, D, B=B), f"v2(seed={seed},B={B},W={W},D={D})")
    assert case is not None, "v2_case_long state without candidates"
    return case


def tone_step(oracle, seed, B=None, W=None, C=None):
    c = dc.tone_case(seed, B=B, W=W, C=C)
    B, W, C = c["h"].shape
    o = oracle.tone_step(c["h"], c["hist"], c["fin"], c["t"], c["u"], c["input_length"],
                         c["empty_tone_id"])
    want = [o[k] for k in V1_KEYS]
    return Case(f"tone(seed={seed},B={B},W={W},C={C})",
                lambda capi: capi.tone_latent_beam_search_decode(
                    c["h"], c["hist"], c["fin"], c["t"], c["u"], c["input_length"], B, W, C,
                    c["empty_tone_id"]),
                want, _nbytes(c["h"], c["hist"], c["fin"], c["t"], c["u"], c["input_length"], *want))


def order(oracle, B, W, T, seed=0):
    rng = np.random.default_rng(seed + 6000)
    bb = rng.integers(0, W, size=(B, T, W)).astype(np.int32)
    fb = rng.integers(0, W, size=(B, W)).astype(np.int32)
    want = oracle.order_beam_branch(fb, bb)
    return Case(f"order(B={B},W={W},T={T})",
                lambda capi: [capi.ssnt_order_beam_branch(fb, bb, B, W, T)],
                [want], _nbytes(fb, bb, want))


def upsample(oracle, B, W, max_t, max_u, seed=0):
    """Durations 0..5, one row all zero (output_length 0); the caller's array arrives prefilled
    with a different value in every element, and every element at or past its row's
    output_length must come back as sent."""
    rng = np.random.default_rng(seed + 7000)
    d = rng.integers(0, 6, size=(B, W, max_t)).astype(np.int32)
    d[0, 0, :] = 0
    ol = d.sum(-1).astype(np.int32)
    assert 0 < ol.max() <= max_u
    prefill = (-5 - np.arange(B * W * max_u, dtype=np.int64)).astype(np.int32).reshape(B, W, max_u)
    o, rc = oracle.upsample_source_indexes(d, ol, max_u)
    assert rc == 0
    written = np.arange(max_u)[None, None, :] < ol[:, :, None]
    want = np.where(written, o, prefill).astype(np.int32)
    assert (want[written] >= 0).all() and (want[~written] < 0).all()
    return Case(f"upsample(B={B},W={W},T={max_t},U={max_u})",
                lambda capi: [capi.ssnt_upsample_source_indexes(d, ol, B, W, max_t, max_u,
                                                                out=prefill.copy())],
                [want], _nbytes(d, ol, want))


def edit_distance(oracle, B, L, seed=0):
    """Ragged lengths; 0 and L both occur on either side."""
    rng = np.random.default_rng(seed + 8000)
    a = rng.integers(0, 5, size=(B, L)).astype(np.int32)
    b = rng.integers(0, 5, size=(B, L)).astype(np.int32)
    al = rng.integers(0, L + 1, size=B).astype(np.int32)
    bl = rng.integers(0, L + 1, size=B).astype(np.int32)
    al[0], bl[0] = L, L
    if B > 2:
        al[1], bl[1], al[2], bl[2] = 0, L, L, 0
    want = oracle.levenshtein(a, b, al, bl)
    return Case(f"edit(B={B},L={L})",
                lambda capi: [capi.tone_latent_levenshtein_edit_distance(a, b, al, bl, B, L)],
                [want], _nbytes(a, b, al, bl, want))


def extract(oracle, W, max_u, seed=0):
    rng = np.random.default_rng(seed + 9000)
    bb = rng.integers(0, W, size=(max_u, W)).astype(np.int32)
    th = rng.integers(0, 1000, size=(max_u, W)).astype(np.int32)
    best = int(rng.integers(0, W))
    want = oracle.extract_best_beam_branch(best, bb, th)
    return Case(f"extract(W={W},U={max_u})",
                lambda capi: capi.ssnt_extract_best_beam_branch(best, bb, th, W, max_u),
                want, _nbytes(bb, th, *want) + 4)


def lattice_inputs(oracle, B, T, U, seed, infeasible=None):
    """log_trans, log_obs, ragged step_len / pos_len with a full-size utterance first; utterance
    `infeasible` has more positions than steps (no path: loss 0 under zero_infinity)."""
    rng = np.random.default_rng(seed + 10000)
    lt = oracle.synth_log_trans(B, T, U, seed=seed)
    lo = (rng.standard_normal((B, T, U)) * 3 - 5).astype(np.float32)
    P = np.array([U] + [int(x) for x in rng.integers(1, U + 1, size=B - 1)], np.int32)
    S = np.array([T] + [int(rng.integers(min(p, T), T + 1)) for p in P[1:]], np.int32)
    if infeasible is not None:
        S[infeasible], P[infeasible] = min(5, T), U
    return lt, lo, S, P


def fwd_bwd(oracle, B, T, U, seed=0, obs=True, debug=True):
    """The host-pointer forward-backward through capi.ssnt_fwd_bwd (every output it has)."""
    lt, lo, S, P = lattice_inputs(oracle, B, T, U, seed)
    lo = lo if obs else None
    o = oracle.fwd_bwd_xf(lt, S, P, log_obs=lo, debug=debug)
    keys = [k for k in FB_KEYS if k in o]

    def call(capi):
        r = capi.ssnt_fwd_bwd(lt, S, P, log_obs=lo, debug=debug)
        return [r[k] for k in keys]
    return Case(f"fwd_bwd(B={B},T={T},U={U},obs={int(obs)},debug={int(debug)})", call,
                [o[k] for k in keys], _nbytes(lt, S, P, *( [lo] if obs else []), *[o[k] for k in keys]))
