"""GPU best duration path on the v2 lattice (v2_viterbi.hip) against the
numpy-f32 DP of tests/v2_viterbi_ref.py: log_prob bit-identical (tobytes), duration_class,
duration and total value-identical (np.array_equal), on both cell forms, every class padding,
both backpointer stores (LDS, workspace), tie-rich and edge inputs, at the configs[4] shape
against a planted path, plus invariants that do not use the DP, the round trip through
upsample_source_indexes, and the API / error paths."""
import functools

import numpy as np
import pytest
import torch

import f4_cases
import guarded as G
import v2_viterbi_ref as VR
from gpu_util import DEV, poisoned_runs, switch_point, _t, vp

pytestmark = pytest.mark.gpu

KEYS = ("duration_class", "duration", "total")


def _run(gpu, logits, table, I, O, max_total, zid=0, allow_skip=True, test_mode=False, **kw):
    r = gpu.v2_viterbi_align(_t(np.asarray(logits, np.float32)), _t(np.asarray(table), torch.int32),
                             _t(np.asarray(I), torch.int32), _t(np.asarray(O), torch.int32), zid,
                             allow_skip=allow_skip, test_mode=test_mode, max_total=max_total, **kw)
    return {k: v.cpu().numpy() for k, v in r.items()}


def _same(g, ref, where=""):
    assert g["log_prob"].dtype == np.float32
    assert g["log_prob"].tobytes() == ref["log_prob"].tobytes(), (where, g["log_prob"], ref["log_prob"])
    for k in KEYS:
        assert g[k].dtype == np.int32 and np.array_equal(g[k], ref[k]), (where, k)


def _check_empty(g, b):
    assert np.isneginf(g["log_prob"][b]) and g["total"][b] == -1
    assert np.all(g["duration_class"][b] == -1) and np.all(g["duration"][b] == 0)


def _softmax_logits(rng, shape):
    z = rng.standard_normal(shape).astype(np.float32) * np.float32(1.5)
    m = z.max(-1, keepdims=True)
    return (z - (m + np.log(np.exp(z - m).sum(-1, keepdims=True)))).astype(np.float32)


# ---- 1. small cases --------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("mode", VR.MODES)
def test_small_bit_exact(gpu, seed, mode):
    B, Imax, D = 7, 9, 5
    logits, I, O = f4_cases.random_case(np.random.default_rng(seed), B, Imax, D)
    table = np.arange(D, dtype=np.int32)
    test_mode, allow_skip = mode == "test_mode", mode != "no_skip"
    mt = int(O.max()) + (9 if test_mode else 0)
    g = _run(gpu, logits, table, I, O, mt, 0, allow_skip, test_mode, check=True)
    _same(g, VR.dp(logits, table, I, O, mt, 0, allow_skip, test_mode))


@pytest.mark.parametrize("mode", VR.MODES)
def test_brute_force_cases(gpu, mode):
    feasible = 0
    for seed in range(6):
        case = VR.tiny_case(seed, mode)
        logits, table, I, O, mt, allow_skip, test_mode = case
        g = _run(gpu, logits, table, I, O, mt, 0, allow_skip, test_mode, check=True)
        f, _ = VR.check_against_brute_force(g, case, VR.case_brute_force("tiny", seed, mode))
        feasible += f
    assert feasible >= 36, feasible  # half of the mode's 72 utterances


# ---- 2. medium ragged ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _medium(oracle, test_mode):
    B, Imax, D = 12, 60, 8  # the generator of test_gpu_v2_fwd_bwd.py::test_medium_ragged_bit_exact
    d = oracle.synth_durations(B, Imax, 4 * Imax, D, seed=3)
    logits = oracle.synth_v2_step_logits(d, D, seed=4)
    rng = np.random.default_rng(5)
    I = rng.integers(Imax // 2, Imax + 1, size=B).astype(np.int32)
    I[0] = Imax
    O = np.array([int(d[b, :I[b]].sum()) for b in range(B)], np.int32)
    table = np.arange(D, dtype=np.int32)
    mt = int(O.max()) + (40 if test_mode else 3)
    return logits, table, I, O, mt


@pytest.mark.parametrize("test_mode", [False, True])
def test_medium_ragged_bit_exact(gpu, oracle, test_mode):
    logits, table, I, O, mt = _medium(oracle, test_mode)
    g = _run(gpu, logits, table, I, O, mt, 0, True, test_mode, check=True)
    _same(g, VR.dp(logits, table, I, O, mt, 0, True, test_mode))
    assert np.all(g["log_prob"] > -np.inf)


# ---- 3. duration tables: both cell forms, every class padding, more than two weight chunks ----
F4_TABLES = [  # = test_gpu_v2_fwd_bwd.py
    ("long_durations", [0, 3, 70, 5, 100, 2]),  # dmax 100 > 64: the clamped cell form
    ("shuffled16", [7, 0, 12, 3, 9, 1, 15, 4, 2, 11, 6, 14, 8, 13, 10, 5]),
    ("d20", list(range(0, 60, 3))),              # 32 class slots
    ("d40", [(5 * i) % 64 for i in range(40)]),  # 64 class slots, 32-step weight chunks
]


@pytest.mark.parametrize("test_mode", [False, True])
@pytest.mark.parametrize("name,table", F4_TABLES, ids=[t[0] for t in F4_TABLES])
def test_duration_tables_bit_exact(gpu, name, table, test_mode):
    table = np.array(table, np.int32)
    D = len(table)
    B, Imax = 5, 150
    rng = np.random.default_rng(D)
    logits = _softmax_logits(rng, (B, Imax, D))
    I = np.array([150, 149, 97, 70, 20], np.int32)
    O = np.array([int(table[rng.integers(0, D, size=i)].sum()) for i in I], np.int32)
    O[4] = int(I[4]) * (int(table.max()) + 30)  # a band that moves further per step than dmax
    mt = int(O[:4].max()) + (7 if test_mode else 0)
    if test_mode:
        O[4] = min(int(O[4]), mt)
    g = _run(gpu, logits, table, I, O, mt, 0, True, test_mode, check=True)
    _same(g, VR.dp(logits, table, I, O, mt, 0, True, test_mode), name)
    assert np.isfinite(g["log_prob"][:4]).any()


# ---- 4. edges --------------------------------------------------------------------------------
def _edge_inputs():
    rng = np.random.default_rng(11)  # the inputs of test_gpu_v2_fwd_bwd.py::test_edges
    logits, _, _ = f4_cases.random_case(rng, 7, 6, 4)
    table = np.array([0, 1, 2, 3], np.int32)
    I = np.array([6, 0, 4, 6, 3, 6, 5], np.int32)
    O = np.array([19, 5, 9, 16, 6, 14, 12], np.int32)  # > max_total, I=0, ok, no moves, ok, overrun, ok
    logits[3] = -np.inf
    logits[6, 2, :2] = np.nan  # NaN log-probs never win
    logits[4, 1, 1] = np.inf   # not clamped: follows the recurrence
    return logits, table, I, O


def test_edges(gpu):
    logits, table, I, O = _edge_inputs()
    ref = VR.dp(logits, table, I, O, 18, 0, True, False)
    g = _run(gpu, logits, table, I, O, 18, 0, True, False, check=True)
    _same(g, ref)
    for b in (0, 1, 3, 5):
        _check_empty(g, b)
    assert np.all(g["log_prob"][[2, 6]] > -np.inf)
    assert not np.isnan(g["log_prob"]).any()


def test_bad_length_and_bad_table_status(gpu):
    logits, table, I, O = _edge_inputs()
    lib = gpu.load()
    I2 = I.copy()
    I2[2] = 7  # > max_steps
    g = _run(gpu, logits, table, I2, O, 18)
    _same(g, VR.dp(logits, table, I2, O, 18, 0, True, False))
    _check_empty(g, 2)
    assert g["log_prob"][6] > -np.inf
    assert lib.ssnt_status_from_bits(int(g["status"][0])) == 7  # SSNT_ERR_BAD_LENGTH
    with pytest.raises(gpu.SsntError) as e:
        _run(gpu, logits, table, I2, O, 18, check=True)
    assert e.value.code == 7
    O2 = O.copy()
    O2[4] = -1
    g = _run(gpu, logits, table, I, O2, 18)
    _check_empty(g, 4)
    assert lib.ssnt_status_from_bits(int(g["status"][0])) == 7
    bad = np.array([0, 1, -2, 3], np.int32)  # a negative entry: every utterance infeasible
    g = _run(gpu, logits, bad, I, O, 18)
    _same(g, VR.dp(logits, bad, I, O, 18, 0, True, False))
    for b in range(7):
        _check_empty(g, b)
    assert lib.ssnt_status_from_bits(int(g["status"][0])) == 8  # SSNT_ERR_BAD_INDEX


# ---- 5. ties ---------------------------------------------------------------------------------
@pytest.mark.parametrize("test_mode", [False, True])
def test_tie_rich(gpu, test_mode):
    B, Imax, D = 8, 40, 6
    rng = np.random.default_rng(40 + test_mode)
    table = np.array([0, 3, 4, 3, 5, 4], np.int32)  # two pairs of classes with equal durations
    logits = rng.choice(np.array([-0.5, -1.0, -1.5], np.float32), size=(B, Imax, D))
    logits[0] = -1.0  # one all-equal utterance: every admissible sequence ties
    I = rng.integers(10, Imax + 1, size=B).astype(np.int32)
    I[0] = Imax
    O = np.array([int(rng.integers(3 * i, 5 * i + 1)) for i in I], np.int32)  # (no overrun: O >= 3 I)
    mt = int(O.max()) + (5 if test_mode else 0)
    ref = VR.dp(logits, table, I, O, mt, 0, True, test_mode)
    assert np.all(ref["log_prob"] > -np.inf)
    _same(_run(gpu, logits, table, I, O, mt, 0, True, test_mode, check=True), ref)
    for tm in (False, True):  # and the brute-force tie set of the CPU file
        for seed in range(6):
            case = VR.tie_case(seed, tm)
            lg, tb, Ic, Oc, mtc, sk, _ = case
            g = _run(gpu, lg, tb, Ic, Oc, mtc, 0, sk, tm, check=True)
            VR.check_against_brute_force(g, case, VR.case_brute_force("tie", seed, tm))
            _same(g, VR.dp(lg, tb, Ic, Oc, mtc, 0, sk, tm), ("tie set", seed, tm))


# ---- 6. backpointer stores -------------------------------------------------------------------
def _switch_I(gpu, max_total, test_mode):
    """The largest max_steps whose backpointers stay in LDS (by the size query)."""
    q = gpu.load().ssnt_v2_viterbi_align_workspace_size
    return switch_point(lambda I: q(1, I, max_total, test_mode), hi=1 << 20)


def _poisoned(gpu, logits, table, I, O, mt, test_mode):
    """The C entry with a workspace of exactly the queried size in a guarded arena (guarded.py),
    filled with 0xFF, with 0x00, and left as a finished run of other logits of the same shape
    wrote it: the results of the three runs (the guards are checked after each)."""
    lib = gpu.load()
    B, T, D = logits.shape
    need = int(lib.ssnt_v2_viterbi_align_workspace_size(B, T, mt, test_mode))
    assert need > 0
    f32, i32 = torch.float32, torch.int32
    arena, v = G.lay_out(DEV, {"lg": ((B, T, D), f32), "table": ((D,), i32), "il": ((B,), i32),
                               "ol": ((B,), i32), "log_prob": ((B,), f32), "duration_class": ((B, T), i32),
                               "duration": ((B, T), i32), "total": ((B,), i32), "status": ((1,), i32),
                               "ws": ((need,), torch.uint8)})
    for k, a in (("table", table), ("il", I), ("ol", O)):
        G.put(v[k], np.asarray(a, np.int32))

    def call():
        return G.call(lib, "ssnt_v2_viterbi_align_device", v["lg"], v["table"], v["il"], v["ol"], B, T, D,
                      int(mt), 0, True, bool(test_mode), v["log_prob"], v["duration_class"], v["duration"],
                      v["total"], v["ws"], need, v["status"], torch.cuda.current_stream().cuda_stream)

    return poisoned_runs(arena, v, lambda x: G.put(v["lg"], np.ascontiguousarray(x, np.float32)), call, logits,
                         logits[::-1, ::-1], ("log_prob", "duration_class", "duration", "total"))


@pytest.mark.parametrize("test_mode,mt", [(True, 300), (False, 2000)], ids=["test_mode", "band"])
def test_lds_to_workspace_switch(gpu, oracle, test_mode, mt):
    q = gpu.load().ssnt_v2_viterbi_align_workspace_size
    assert q(64, 400, 2000, True) > 0  # test mode at the configs[4] shape: the workspace side
    assert q(64, 400, 2000, False) == 0
    Il = _switch_I(gpu, mt, test_mode)
    assert 100 < Il < 1000, Il
    B, D = 2, 8
    table = np.arange(D, dtype=np.int32)
    for T in (Il, Il + 1):
        I = np.array([T, T - 70], np.int32)
        if test_mode:
            O = np.array([mt, mt - 5], np.int32)
            logits = _softmax_logits(np.random.default_rng(T), (B, T, D))
        else:  # a path that sums to O inside the band exists
            O = np.array([mt, (mt * (T - 70)) // T], np.int32)
            d = oracle.synth_durations(B, I, O, D, seed=T)
            logits = oracle.synth_v2_step_logits(d, D, seed=T + 1, margin=1.0)
        ref = VR.dp(logits, table, I, O, mt, 0, True, test_mode)
        assert np.all(ref["log_prob"] > -np.inf)
        _same(_run(gpu, logits, table, I, O, mt, 0, True, test_mode, check=True), ref, T)
        if q(B, T, mt, test_mode) > 0:
            for g in _poisoned(gpu, logits, table, I, O, mt, test_mode):
                _same(g, ref, (T, "poisoned"))
    assert q(B, Il, mt, test_mode) == 0 and q(B, Il + 1, mt, test_mode) > 0


# ---- 7. the configs[4] shape ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _config5(oracle, margin=3.0):
    B, I, Ot, D = 64, 400, 2000, 16  # the inputs of test_gpu_v2_fwd_bwd.py::test_config5_bit_exact
    d = oracle.synth_durations(B, I, Ot, D, seed=0)
    logits = oracle.synth_v2_step_logits(d, D, seed=1, margin=margin)
    return logits, np.arange(D, dtype=np.int32), np.full(B, I, np.int32), np.full(B, Ot, np.int32), Ot, d


@functools.lru_cache(maxsize=None)
def _config5_dp(oracle, test_mode):
    logits, table, il, ol, Ot, _ = _config5(oracle)
    return VR.dp(logits, table, il, ol, Ot, 0, False, test_mode)


@pytest.mark.parametrize("test_mode", [False, True])
def test_config5_bit_exact(gpu, oracle, test_mode):
    logits, table, il, ol, Ot, _ = _config5(oracle)
    g = _run(gpu, logits, table, il, ol, Ot, 0, False, test_mode, check=True)
    _same(g, _config5_dp(oracle, test_mode))
    assert np.all(np.isfinite(g["log_prob"]))


@pytest.mark.parametrize("test_mode", [False, True])
def test_config5_recovers_the_planted_path(gpu, oracle, test_mode):
    # margin 12: the planted class outweighs every detour, so the best path is the planted one
    # (a known answer that does not come from the DP)
    logits, table, il, ol, Ot, d = _config5(oracle, 12.0)
    g = _run(gpu, logits, table, il, ol, Ot, 0, False, test_mode, check=True)
    assert np.array_equal(g["duration"], d)
    assert np.array_equal(g["duration_class"], d)  # duration_table = [0..15]
    assert np.all(g["total"] == Ot)


# ---- 8. invariants that do not use the DP ----------------------------------------------------
@pytest.mark.parametrize("test_mode", [False, True])
def test_path_invariants(gpu, oracle, test_mode):
    logits, table, I, O, mt = _medium(oracle, test_mode)
    g = _run(gpu, logits, table, I, O, mt, 0, True, test_mode, check=True)
    f64 = oracle.v2_fwd_bwd_f64(logits, table, I, O, mt, 0, True, test_mode)["loss"]
    for b in range(len(I)):
        n = int(I[b])
        cls, dur = g["duration_class"][b, :n], g["duration"][b, :n]
        assert np.all(cls >= 0) and np.array_equal(dur, table[cls])
        assert int(dur.sum()) == int(g["total"][b])
        pre = np.cumsum(dur)
        if test_mode:
            assert pre[-1] <= mt
        else:
            assert pre[-1] == O[b]
            for t in range(n):
                lb, ub = f4_cases.band(t, n, int(O[b]))
                assert lb <= pre[t] <= ub, (b, t)
        v32, v64 = np.float32(0), 0.0
        for t in range(n):
            v32, v64 = np.float32(v32 + logits[b, t, cls[t]]), v64 + float(logits[b, t, cls[t]])
        assert np.float32(v32).tobytes() == g["log_prob"][b].tobytes()
        assert v64 <= -f64[b] + 1e-9 * max(1.0, abs(f64[b]))  # one path never outweighs Z


def test_config5_not_below_the_beam(gpu, oracle):
    # the exact best path is at least as probable as the path a W=4 beam keeps in slot 0 (4 ulps:
    # the beam sums the same terms in another order)
    logits, table, il, ol, Ot, _ = _config5(oracle)
    g = _run(gpu, logits, table, il, ol, Ot, 0, False, False, check=True)
    W = 4
    lg4 = _t(logits)[:, :, None, :].expand(-1, -1, W, -1).contiguous()
    d = gpu.v2_lattice_beam_search_decode(lg4, _t(table), _t(il), _t(ol), W, 0, False, False, check=False)
    beam = d["log_prob"][:, -1, 0].cpu().numpy()
    tot = d["next_total_duration"][:, -1, 0].cpu().numpy()
    ok = np.isfinite(beam) & (tot == Ot)  # a beam that lost every admissible path has no answer
    assert ok.sum() >= 32, int(ok.sum())
    assert np.all(g["log_prob"][ok] >= beam[ok] - 4 * np.spacing(np.abs(beam[ok])))


# ---- 9. round trip through upsample_source_indexes --------------------------------------------
def test_round_trip_through_upsample(gpu, oracle):
    logits, table, I, O, mt = _medium(oracle, False)
    r = gpu.v2_viterbi_align(_t(logits), _t(table), _t(I), _t(O), 0, allow_skip=True, max_total=mt,
                             check=True)
    up = gpu.upsample_source_indexes(r["duration"][:, None, :], r["total"][:, None], -1, 1)[:, 0]
    up, dur = up.cpu().numpy(), r["duration"].cpu().numpy()
    for b in range(len(I)):
        want = np.repeat(np.arange(int(I[b])), dur[b, :I[b]])
        assert np.array_equal(up[b, :len(want)], want)
        assert np.all(up[b, len(want):] == -1)


# ---- 10. API, error paths, streams -----------------------------------------------------------
def test_need_path_false_and_out_reuse(gpu, oracle):
    logits, table, I, O, mt = _medium(oracle, False)
    B, T, _ = logits.shape
    ref = VR.dp(logits, table, I, O, mt, 0, True, False)
    n = _run(gpu, logits, table, I, O, mt, need_path=False, check=True)
    assert set(n) == {"log_prob", "status"}
    assert n["log_prob"].tobytes() == ref["log_prob"].tobytes()
    out = {"log_prob": torch.full((B,), 7.0, device=DEV),
           "duration_class": torch.full((B, T), 9, dtype=torch.int32, device=DEV),
           "duration": torch.full((B, T), 9, dtype=torch.int32, device=DEV),
           "total": torch.full((B,), 9, dtype=torch.int32, device=DEV),
           "status": torch.ones(1, dtype=torch.int32, device=DEV)}
    args = (_t(logits), _t(table), _t(I), _t(O), 0)
    r = gpu.v2_viterbi_align(*args, allow_skip=True, max_total=mt, out=out, check=True)
    for k in out:
        assert r[k].data_ptr() == out[k].data_ptr()
    _same({k: v.cpu().numpy() for k, v in r.items()}, ref)
    d = gpu.v2_viterbi_align(*args, allow_skip=True, check=True)  # max_total defaults to max(O)
    _same({k: v.cpu().numpy() for k, v in d.items()}, VR.dp(logits, table, I, O, int(O.max()), 0, True, False))
    with pytest.raises(ValueError):
        gpu.v2_viterbi_align(*args, out={"duration": torch.empty((B, T), dtype=torch.int64, device=DEV)})
    with pytest.raises(ValueError):
        gpu.v2_viterbi_align(*args, out={"total": torch.empty((B + 1,), dtype=torch.int32, device=DEV)})


def test_error_returns(gpu):
    lib = gpu.load()
    B, T, D, mt = 2, 6, 4, 12
    x = torch.zeros((B, T, D), device=DEV)
    tb = torch.arange(D, dtype=torch.int32, device=DEV)
    il = torch.full((B,), T, dtype=torch.int32, device=DEV)
    ol = torch.full((B,), mt, dtype=torch.int32, device=DEV)
    lp = torch.empty(B, device=DEV)
    st = torch.zeros(1, dtype=torch.int32, device=DEV)

    def call(lg=x, table=tb, i=il, o=ol, b=B, t=T, d=D, m=mt, test=False, out=lp, cls=None, ws=None, wsb=0):
        return lib.ssnt_v2_viterbi_align_device(vp(lg), vp(table), vp(i), vp(o), b, t, d, m, 0, True, test,
                                                vp(out), vp(cls), None, None, vp(ws), wsb, vp(st), None)

    INVALID, UNSUPPORTED, WORKSPACE = 1, 5, 6
    assert call() == 0
    assert call(lg=None) == INVALID and call(table=None) == INVALID and call(i=None) == INVALID
    assert call(o=None) == INVALID and call(out=None) == INVALID
    assert call(b=-1) == INVALID and call(t=0) == INVALID and call(d=0) == INVALID
    assert call(m=-1) == INVALID and call(m=(1 << 24) + 1) == INVALID
    assert call(d=65) == UNSUPPORTED
    assert call(m=1 << 24, test=True) == UNSUPPORTED  # a row beyond LDS
    assert call(b=0, lg=None, out=None) == 0
    # a shape whose backpointers need the workspace: missing / one byte short; none without a path
    Tw, mw = 500, 400
    need = int(lib.ssnt_v2_viterbi_align_workspace_size(1, Tw, mw, True))
    assert need > 0
    big = torch.zeros((1, Tw, D), device=DEV)
    one = torch.full((1,), Tw, dtype=torch.int32, device=DEV)
    cls = torch.empty((1, Tw), dtype=torch.int32, device=DEV)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    kw = dict(lg=big, i=one, o=one, b=1, t=Tw, m=mw, test=True)
    assert call(cls=cls, **kw) == WORKSPACE
    assert call(cls=cls, ws=ws, wsb=need - 1, **kw) == WORKSPACE
    assert call(cls=cls, ws=ws, wsb=need, **kw) == 0
    assert call(**kw) == 0
    torch.cuda.synchronize()
    assert int(st.item()) == 0


def test_two_streams(gpu):
    B, T, D, mt = 3, 500, 8, 400  # a workspace shape: each call owns its workspace
    assert gpu.load().ssnt_v2_viterbi_align_workspace_size(B, T, mt, True) > 0
    table = np.arange(D, dtype=np.int32)
    a = _softmax_logits(np.random.default_rng(1), (B, T, D))
    b = _softmax_logits(np.random.default_rng(2), (B, T, D))
    I, O = np.array([T, T - 9, T - 100], np.int32), np.full(B, mt, np.int32)
    ra, rb = (VR.dp(x, table, I, O, mt, 0, True, True) for x in (a, b))
    assert not np.array_equal(ra["duration_class"], rb["duration_class"])
    xa, xb, tb = _t(a), _t(b), _t(table)
    il, ol = _t(I), _t(O)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        ga = gpu.v2_viterbi_align(xa, tb, il, ol, 0, allow_skip=True, test_mode=True, max_total=mt)
    with torch.cuda.stream(s2):
        gb = gpu.v2_viterbi_align(xb, tb, il, ol, 0, allow_skip=True, test_mode=True, max_total=mt)
    torch.cuda.synchronize()
    _same({k: v.cpu().numpy() for k, v in ga.items()}, ra, "stream 1")
    _same({k: v.cpu().numpy() for k, v in gb.items()}, rb, "stream 2")
