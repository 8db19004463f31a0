"""GPU posterior sampling on the v2 duration-class lattice (v2_sample_align.hip, DESIGN.md 2.5 /
5.9) against the float64 reference of tests/v2_sample_ref.py. The uniforms are an input, so every
sample the reference calls clear (margin > DELTA) must come out with exactly its classes and total;
every sample, clear or not, must be an admissible sequence (f4_cases.move_ok per move) whose
log_prob is the sequential f32 sum of its class log-probs, bit for bit, and no larger than the
best path's (v2_viterbi_align). Plus frequencies against the enumerated posterior, the infeasible
rule, the clamp, every refusal, a poisoned workspace, the Python surface and two streams."""
import numpy as np
import pytest
import torch

import f4_cases
import guarded as G
import v2_sample_ref as SR
import v2_viterbi_ref as VR
from gpu_util import DEV, poisoned_runs, _t, vp

pytestmark = pytest.mark.gpu

OUT_KEYS = ("log_prob", "duration_class", "duration", "total")


def _args(case):
    logits, table, I, O, mt, allow_skip, test_mode = case
    return ((_t(np.asarray(logits, np.float32)), _t(np.asarray(table), torch.int32), _t(np.asarray(I), torch.int32),
             _t(np.asarray(O), torch.int32), 0), dict(allow_skip=allow_skip, test_mode=test_mode, max_total=mt))


def _run(gpu, case, K, u, **kw):
    args, mode = _args(case)
    r = gpu.v2_sample_align(*args, K, uniform=None if u is None else _t(np.asarray(u, np.float32)), **mode, **kw)
    return {k: v.cpu().numpy() for k, v in r.items()}


def _best(gpu, case):
    args, mode = _args(case)
    return gpu.v2_viterbi_align(*args, need_path=False, **mode)["log_prob"].cpu().numpy()


def _check_empty(g, b):
    assert np.all(np.isneginf(g["log_prob"][b])) and np.all(g["total"][b] == -1)
    assert np.all(g["duration_class"][b] == -1) and np.all(g["duration"][b] == 0)


def _check(gpu, case, g, ref=None):
    """What every case must satisfy; with `ref` (v2_sample_ref.sample_batch / clear_uniforms) also
    the feasibility and every clear sample. Returns the number of clear samples compared."""
    logits, table, I, O, mt, allow_skip, test_mode = case
    B, T, _ = logits.shape
    K = g["log_prob"].shape[1]
    X = mt + 1
    best = _best(gpu, case)
    for k in OUT_KEYS:
        assert g[k].dtype == (np.float32 if k == "log_prob" else np.int32), k
    for b in range(B):
        if g["total"][b, 0] < 0:
            _check_empty(g, b)
            assert np.isneginf(best[b])
            continue
        n = int(I[b])
        for k in range(K):
            cls, dur = g["duration_class"][b, k], g["duration"][b, k]
            assert np.all(cls[:n] >= 0) and np.all(cls[n:] == -1) and np.all(dur[n:] == 0), (b, k)
            assert np.array_equal(dur[:n], np.asarray(table)[cls[:n]]), (b, k)
            tot = 0
            for t in range(n):
                tot += int(table[cls[t]])
                assert f4_cases.move_ok(t, tot, int(cls[t]), n, int(O[b]), X, 0, allow_skip, test_mode), (b, k, t)
            assert tot == int(g["total"][b, k]) == int(dur.sum()), (b, k)
            if not test_mode:
                assert tot == int(O[b])
            lp = g["log_prob"][b, k]
            assert lp.tobytes() == SR.path_log_prob_f32(logits[b], cls).tobytes(), (b, k)
            assert lp <= best[b], (b, k, lp, best[b])  # exact: the f32 add is monotone
    if ref is None:
        return 0
    assert np.array_equal(g["total"][:, 0] >= 0, ref["feasible"])
    clear = SR.clear(ref)
    for b, k in zip(*np.nonzero(clear)):
        assert np.array_equal(g["duration_class"][b, k], ref["duration_class"][b, k]), (b, k)
        assert g["total"][b, k] == ref["total"][b, k], (b, k)
    return int(clear.sum())


# ---- 1. the case families: tiny in all modes, the duration tables, the three walk forms --------
@pytest.mark.parametrize("name", sorted(SR.FAMILIES))
def test_family_clear_samples_equal_the_reference(gpu, name):
    case, K, u, ref = SR.family(name)
    g = _run(gpu, case, K, u, check=True)
    n = _check(gpu, case, g, ref)
    assert n >= 0.99 * int(ref["feasible"].sum()) * K


# ---- 2. a window wider than 512 cells, a final-total CDF longer than one wave -------------------
def test_wide_window_and_final_totals(gpu):
    B, T, D, K = 2, 45, 16, 8
    logits = np.log(np.random.default_rng(3).dirichlet(np.ones(D), size=(B, T))).astype(np.float32)
    case = (logits, np.arange(D, dtype=np.int32), np.array([45, 44], np.int32), np.array([300, 320], np.int32),
            700, True, True)
    u, ref = SR.clear_uniforms(case, K, 1)
    g = _run(gpu, case, K, u, check=True)
    assert _check(gpu, case, g, ref) >= 15
    assert len(np.unique(g["total"][0])) >= 2 and g["total"].max() > 64


# ---- 3. sample-count extremes -----------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 63, 64])
def test_sample_count_edges(gpu, K):
    B, Imax, D = 3, 9, 5
    logits, I, O = f4_cases.random_case(np.random.default_rng(K), B, Imax, D)
    case = (logits, np.arange(D, dtype=np.int32), I, O, int(O.max()) + 9, True, True)
    u, ref = SR.clear_uniforms(case, K, 2)
    g = _run(gpu, case, K, u, check=True)
    assert g["log_prob"].shape == (B, K) and g["duration_class"].shape == (B, K, Imax)
    assert _check(gpu, case, g, ref) >= 0.99 * B * K


# ---- 4. frequencies against the enumerated posterior -------------------------------------------
def test_frequencies_match_the_posterior(gpu):
    B, K, I, D = 128, 64, 5, 4
    lg1, _, _ = f4_cases.random_case(np.random.default_rng(21), 1, I, D)
    table = np.array([0, 1, 2, 3], np.int32)
    case = (np.repeat(lg1, B, 0), table, np.full(B, I, np.int32), np.full(B, 8, np.int32), 11, True, True)
    u = np.random.default_rng(22).random((B, K, I + 1), dtype=np.float32)
    g = _run(gpu, case, K, u, check=True)
    post = SR.path_posterior(lg1[0], table, I, 8, 11, 0, True, True)
    assert len(post) > 100
    dev = SR.frequency_deviation(g["duration_class"].reshape(B * K, I), g["total"].reshape(B * K), I, post)
    assert dev <= 5.0, dev
    two = (case[0][:2], table, case[2][:2], case[3][:2], 11, True, True)
    _check(gpu, two, {k: g[k][:2] for k in OUT_KEYS})


# ---- 5. the exponent range of the long-form shape ---------------------------------------------
def test_long_form_exponent_range(gpu):
    B, I, Ot, D, K = 2, 400, 2000, 16, 4
    logits = np.log(np.random.default_rng(8).dirichlet(np.ones(D), size=(B, I))).astype(np.float32)
    case = (logits, np.arange(D, dtype=np.int32), np.full(B, I, np.int32), np.full(B, Ot, np.int32), Ot,
            False, False)
    u, ref = SR.clear_uniforms(case, K, 3)
    assert ref["feasible"].all()
    g = _run(gpu, case, K, u, check=True)
    assert np.all(np.isfinite(g["log_prob"])) and np.all(g["log_prob"] < -104)
    assert _check(gpu, case, g, ref) >= 0.99 * B * K


# ---- 6. zero-probability classes are never drawn ------------------------------------------------
def test_zero_probability_classes_are_never_drawn(gpu):
    B, Imax, D, K = 6, 12, 5, 32
    logits, I, O = f4_cases.random_case(np.random.default_rng(31), B, Imax, D)
    logits[:, :, 3] = -np.inf        # one class never
    logits[:, 1::3, :2] = -np.inf    # and two more at every third step
    logits[:, 2, :] = -np.inf
    logits[:, 2, 2] = 0.0            # one step with a single live class
    case = (logits, np.arange(D, dtype=np.int32), I, O, int(O.max()) + 20, True, True)
    u = np.random.default_rng(32).random((B, K, Imax + 1), dtype=np.float32)
    g = _run(gpu, case, K, u, check=True)
    _check(gpu, case, g, SR.sample_batch(case, u))
    assert (g["total"][:, 0] >= 0).all()
    cls = g["duration_class"]
    picked = np.take_along_axis(np.broadcast_to(logits[:, None], (B, K, Imax, D)), np.maximum(cls, 0)[..., None], 3)[..., 0]
    assert np.all(np.isfinite(picked[cls >= 0]))
    assert np.all(np.isfinite(g["log_prob"]))


# ---- 7. edges: the infeasible rule for every sample -------------------------------------------
def _edge_case():
    from test_gpu_v2_viterbi import _edge_inputs
    logits, table, I, O = _edge_inputs()
    logits[np.isnan(logits) | np.isposinf(logits)] = -1.0  # (NaN / +inf inputs are unspecified here)
    return logits, table, I, O, 18, True, False


def test_edges(gpu):
    case = _edge_case()
    K = 5
    u = np.random.default_rng(41).random((7, K, 7), dtype=np.float32)
    g = _run(gpu, case, K, u, check=True)
    ref = SR.sample_batch(case, u)
    _check(gpu, case, g, ref)
    for b in (0, 1, 3, 5):  # O > max_total, I = 0, every logit -inf, overrun
        _check_empty(g, b)
    assert np.all(g["total"][[2, 4, 6]] >= 0)


def test_bad_length_and_bad_table_status(gpu):
    logits, table, I, O, mt, _, _ = _edge_case()
    lib = gpu.load()
    K = 3
    u = np.random.default_rng(42).random((7, K, 7), dtype=np.float32)
    I2 = I.copy()
    I2[2] = 7  # > max_steps
    g = _run(gpu, (logits, table, I2, O, mt, True, False), K, u)
    _check_empty(g, 2)
    assert np.all(g["total"][6] >= 0)
    assert lib.ssnt_status_from_bits(int(g["status"][0])) == 7  # SSNT_ERR_BAD_LENGTH
    with pytest.raises(gpu.SsntError) as e:
        _run(gpu, (logits, table, I2, O, mt, True, False), K, u, check=True)
    assert e.value.code == 7
    O2 = O.copy()
    O2[4] = -1
    g = _run(gpu, (logits, table, I, O2, mt, True, False), K, u)
    _check_empty(g, 4)
    assert lib.ssnt_status_from_bits(int(g["status"][0])) == 7
    bad = np.array([0, 1, -2, 3], np.int32)  # a negative entry: every utterance infeasible
    g = _run(gpu, (logits, bad, I, O, mt, True, False), K, u)
    for b in range(7):
        _check_empty(g, b)
    assert lib.ssnt_status_from_bits(int(g["status"][0])) == 8  # SSNT_ERR_BAD_INDEX
    with pytest.raises(gpu.SsntError) as e:
        _run(gpu, (logits, bad, I, O, mt, True, False), K, u, check=True)
    assert e.value.code == 8


# ---- 8. the clamp -----------------------------------------------------------------------------
def test_uniform_clamp(gpu):
    case = VR.tiny_case(0, "test_mode")
    B, T, _ = case[0].shape
    K = 4

    def run(value):
        g = _run(gpu, case, K, np.full((B, K, T + 1), value, np.float32), check=True)
        _check(gpu, case, g)
        return g

    def same(a, b):
        return all(a[k].tobytes() == b[k].tobytes() for k in OUT_KEYS)

    top, zero = run(SR.U_MAX), run(0.0)
    assert same(run(1.0), top) and same(run(7.0), top)
    assert same(run(np.nan), zero) and same(run(-1.0), zero)
    assert not same(top, zero)
    ref = SR.sample_batch(case, np.full((B, K, T + 1), np.nan, np.float32))  # u = 0: forced, always clear
    assert np.array_equal(zero["duration_class"], ref["duration_class"])


# ---- 9. every refusal: the return code, the outputs and the status word untouched ---------------
def test_refusals_write_nothing(gpu):
    lib = gpu.load()
    B, T, D, mt, K = 2, 6, 4, 15, 3  # (band mode: O >= 3 (I - 1), or the lattice is empty)
    x = torch.zeros((B, T, D), device=DEV)
    tb = torch.arange(D, dtype=torch.int32, device=DEV)
    il = torch.full((B,), T, dtype=torch.int32, device=DEV)
    ol = torch.full((B,), mt, dtype=torch.int32, device=DEV)
    un = torch.full((B, K, T + 1), 0.5, device=DEV)
    need = int(lib.ssnt_v2_sample_align_workspace_size(B, T, mt, False, K))
    assert need > 0
    wsbuf = torch.zeros(need + 16, dtype=torch.uint8, device=DEV)
    assert wsbuf.data_ptr() % 8 == 0
    ws = wsbuf[:need]
    lp = torch.full((B, K), 7.0, device=DEV)
    ints = {k: torch.full(s, 9, dtype=torch.int32, device=DEV)
            for k, s in (("cls", (B, K, T)), ("dur", (B, K, T)), ("tot", (B, K)))}
    st = torch.full((1,), 5, dtype=torch.int32, device=DEV)

    def call(lg=x, table=tb, i=il, o=ol, u=un, b=B, t=T, d=D, m=mt, test=False, k=K, out=lp, w=ws, wsb=need):
        return lib.ssnt_v2_sample_align_device(vp(lg), vp(table), vp(i), vp(o), vp(u), b, t, d, m, 0, True, test, k,
                                               vp(out), vp(ints["cls"]), vp(ints["dur"]), vp(ints["tot"]), vp(w),
                                               wsb, vp(st), None)

    INVALID, UNSUPPORTED, WORKSPACE = 1, 5, 6
    for kw in (dict(k=0), dict(k=65), dict(k=-1), dict(lg=None), dict(table=None), dict(i=None), dict(o=None),
               dict(u=None), dict(out=None), dict(b=-1), dict(t=0), dict(t=-3), dict(d=0), dict(m=-1),
               dict(m=(1 << 24) + 1)):
        assert call(**kw) == INVALID, kw
    assert call(d=65) == UNSUPPORTED
    assert call(m=1 << 24, test=True) == UNSUPPORTED  # a row beyond LDS (F4's limit)
    assert call(w=None) == WORKSPACE and call(w=None, wsb=0) == WORKSPACE
    assert call(wsb=need - 1) == WORKSPACE
    assert call(w=wsbuf.data_ptr() + 4) == WORKSPACE  # misaligned
    assert call(b=0, lg=None, out=None, w=None, wsb=0) == 0
    torch.cuda.synchronize()
    assert torch.all(lp == 7.0) and all(torch.all(v == 9) for v in ints.values())
    assert int(st.item()) == 5
    st.zero_()
    assert call() == 0
    torch.cuda.synchronize()
    assert int(st.item()) == 0 and torch.all(ints["tot"] == mt) and torch.all(torch.isfinite(lp))


# ---- 10. the workspace: exactly the queried size, whatever it held ------------------------------
@pytest.mark.parametrize("test_mode", [False, True])
def test_poisoned_workspace(gpu, test_mode):
    lib = gpu.load()
    name = "i40d16-test_mode" if test_mode else "i40d16-band"
    case, K, u, ref = SR.family(name)
    logits, table, I, O, mt, allow_skip, _ = case
    B, T, D = logits.shape
    need = int(lib.ssnt_v2_sample_align_workspace_size(B, T, mt, test_mode, K))
    f32, i32 = torch.float32, torch.int32
    arena, v = G.lay_out(DEV, {"lg": ((B, T, D), f32), "table": ((D,), i32), "il": ((B,), i32), "ol": ((B,), i32),
                               "un": ((B, K, T + 1), f32), "log_prob": ((B, K), f32),
                               "duration_class": ((B, K, T), i32), "duration": ((B, K, T), i32),
                               "total": ((B, K), i32), "status": ((1,), i32), "ws": ((need,), torch.uint8)})
    for k, a in (("table", table), ("il", I), ("ol", O)):
        G.put(v[k], np.asarray(a, np.int32))
    G.put(v["un"], u)

    def call():
        return G.call(lib, "ssnt_v2_sample_align_device", v["lg"], v["table"], v["il"], v["ol"], v["un"], B, T, D,
                      int(mt), 0, bool(allow_skip), bool(test_mode), K, v["log_prob"], v["duration_class"],
                      v["duration"], v["total"], v["ws"], need, v["status"], torch.cuda.current_stream().cuda_stream)

    res = poisoned_runs(arena, v, lambda x: G.put(v["lg"], np.ascontiguousarray(x, np.float32)), call, logits,
                        logits[::-1, ::-1], OUT_KEYS)
    for r in res[1:]:
        for k in OUT_KEYS:
            assert r[k].tobytes() == res[0][k].tobytes(), k
    _check(gpu, case, res[0], ref)


# ---- 11. the Python surface -------------------------------------------------------------------
def test_python_surface(gpu):
    case, K, u, ref = SR.family("i24d8-band")
    args, mode = _args(case)
    B, T, _ = case[0].shape
    full = _run(gpu, case, K, u, check=True)
    assert set(full) == {"log_prob", "uniform", "status", "duration_class", "duration", "total"}
    n = gpu.v2_sample_align(*args, K, uniform=_t(u), need_path=False, check=True, **mode)
    assert set(n) == {"log_prob", "uniform", "status"}
    assert n["log_prob"].cpu().numpy().tobytes() == full["log_prob"].tobytes()
    out = {"log_prob": torch.full((B, K), 7.0, device=DEV),
           "duration_class": torch.full((B, K, T), 9, dtype=torch.int32, device=DEV),
           "duration": torch.full((B, K, T), 9, dtype=torch.int32, device=DEV),
           "total": torch.full((B, K), 9, dtype=torch.int32, device=DEV),
           "status": torch.ones(1, dtype=torch.int32, device=DEV)}
    r = gpu.v2_sample_align(*args, K, uniform=_t(u), out=out, check=True, **mode)
    for k in out:
        assert r[k].data_ptr() == out[k].data_ptr()
        assert r[k].cpu().numpy().tobytes() == full[k].tobytes(), k
    # generator: the same seed gives the same uniforms and paths; the returned uniforms replay them
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1234)
    a = gpu.v2_sample_align(*args, K, generator=gen, check=True, **mode)
    gen.manual_seed(1234)
    b = gpu.v2_sample_align(*args, K, generator=gen, check=True, **mode)
    c = gpu.v2_sample_align(*args, K, uniform=a["uniform"], check=True, **mode)
    assert tuple(a["uniform"].shape) == (B, K, T + 1) and a["uniform"].dtype == torch.float32
    for k in OUT_KEYS + ("uniform",):
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
    _check(gpu, case, {k: a[k].cpu().numpy() for k in OUT_KEYS})
    d = gpu.v2_sample_align(*args, K, uniform=_t(u), allow_skip=case[5], check=True)  # max_total: max(O)
    assert torch.all(d["total"][torch.from_numpy(ref["feasible"]).to(DEV)] >= 0)
    with pytest.raises(ValueError):
        gpu.v2_sample_align(*args, K, uniform=_t(u[:, :, :-1]), **mode)
    with pytest.raises(ValueError):
        gpu.v2_sample_align(*args, K + 1, uniform=_t(u), **mode)
    with pytest.raises(ValueError):
        gpu.v2_sample_align(*args, K, out={"duration": torch.empty((B, K, T), dtype=torch.int64, device=DEV)}, **mode)
    with pytest.raises(ValueError):
        gpu.v2_sample_align(*args, K, out={"log_prob": torch.empty((B, K), dtype=torch.float64, device=DEV)}, **mode)


# ---- 12. two streams --------------------------------------------------------------------------
def test_two_streams(gpu):
    ca, K, ua, _ = SR.family("table-shuffled16-test_mode")
    cb = (np.ascontiguousarray(ca[0][::-1, ::-1]),) + ca[1:]
    ub = np.ascontiguousarray(ua[::-1])
    ra, rb = _run(gpu, ca, K, ua), _run(gpu, cb, K, ub)
    assert not np.array_equal(ra["duration_class"], rb["duration_class"])
    (xa, mode), (xb, _) = _args(ca), _args(cb)
    ta, tb = _t(ua), _t(ub)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        ga = gpu.v2_sample_align(*xa, K, uniform=ta, **mode)
    with torch.cuda.stream(s2):
        gb = gpu.v2_sample_align(*xb, K, uniform=tb, **mode)
    torch.cuda.synchronize()
    for k in OUT_KEYS:
        assert ga[k].cpu().numpy().tobytes() == ra[k].tobytes(), ("stream 1", k)
        assert gb[k].cpu().numpy().tobytes() == rb[k].tobytes(), ("stream 2", k)
