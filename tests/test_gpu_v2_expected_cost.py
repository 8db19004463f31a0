"""v2_expected_cost on the GPU against the float64 reference (tests/v2_expected_cost_ref.py,
DESIGN.md 2.9): every class-count instantiation, the staging-chunk edges, a window wider than the
workgroup, durations above 64, the modes, infeasible rows, exponent range, cancellation, the
value-only form, exact zeros, the cross-checks against v2_fwd_bwd, the contract (dead rows and
columns, guards, workspace contents, refused calls), determinism and autograd. Errors are
normalised as tests/v2_expected_cost_cases.py `errors` does; the tolerances are 4x the worst value
tools/bench_v2_expected_cost.py --accuracy measured (profiles/v2_expected_cost_accuracy.jsonl, line
"worst"), rounded up to one significant digit."""
import functools

import numpy as np
import pytest
import torch

import contract_cases as CC
import v2_expected_cost_cases as EC
import v2_expected_cost_ref as R
from gpu_util import DEV, _t, vp

pytestmark = pytest.mark.gpu

F32, I32, U8 = torch.float32, torch.int32, torch.uint8
ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE, ERR_BAD_LENGTH, ERR_BAD_INDEX = 1, 5, 6, 7, 8

# 4x profiles/v2_expected_cost_accuracy.jsonl line "worst", one significant digit, rounded up
TOL = {
    "risk": 8e-7,         # worst.errors.risk 1.91e-7 (constant)
    "loss": 9e-7,         # worst.errors.loss 2.13e-7 (wide: absolute, at a loss near 0)
    "grad_logits": 9e-7,  # worst.errors.grad_logits 2.23e-7 (constant)
    "grad_cost": 2e-6,    # worst.errors.grad_cost 4.20e-7 (chunk-4-64)
}
# (the large shape, B=64 I=400 O=2000 D=16, enters "worst" with the first 8 of its 64 utterances
# compared against the float64 reference; its largest value is risk 1.29e-7, entropy cost, band mode)


def _args(c):
    return ((_t(c["logits"]), _t(c["cost"]), _t(c["table"], I32), _t(c["I"], I32), _t(c["O"], I32), c["zid"]),
            dict(allow_skip=c["allow_skip"], test_mode=c["test_mode"], max_total=c["mt"]))


def _run(gpu, c, need_grad=True, out=None, check=False):
    args, mode = _args(c)
    r = gpu.v2_expected_cost(*args, need_grad=need_grad, check=check, out=out, **mode)
    return {k: v.cpu().numpy() for k, v in r.items()}


def _f4(gpu, c):
    r = gpu.v2_fwd_bwd(_t(c["logits"]), _t(c["table"], I32), _t(c["I"], I32), _t(c["O"], I32), c["zid"],
                       allow_skip=c["allow_skip"], test_mode=c["test_mode"], max_total=c["mt"])
    return {k: v.cpu().numpy() for k, v in r.items()}


@functools.lru_cache(maxsize=None)
def _makers():
    import ssnt_tts_amd
    ab = ssnt_tts_amd.load_ab()  # (a host query: no GPU call)
    return EC.case_makers(lambda D: ab.ssnt_v2_expected_cost_chunk_steps(D))


@functools.lru_cache(maxsize=None)
def _case(name):
    return _makers()[name]()


@functools.lru_cache(maxsize=None)
def _ref(name):
    return EC.reference(_case(name))


def _names(prefix):
    # (collected without the A/B library too, e.g. before a build: ssnt_tts_amd.load_ab raises
    # RuntimeError when the file is missing; anything else is a collection error)
    try:
        return [n for n in _makers() if n.startswith(prefix)]
    except RuntimeError:
        return [prefix + "unavailable"]


def _check(got, ref, c, where=""):
    """Every output within tolerance, the exact zeros exact, and the two identities per step."""
    e = EC.errors(got, ref)
    print(where, e)
    for k, v in e.items():
        assert v <= TOL[k], (where, k, v, TOL[k])
    assert int(got["status"][0]) == 0
    for b in range(len(c["I"])):
        n = max(0, min(int(c["I"][b]), c["logits"].shape[1]))
        for k in ("grad_logits", "grad_cost"):
            assert not got[k][b, n:].any(), (where, k, b)  # rows at steps >= I
            if not c["allow_skip"]:
                assert not got[k][b, :, c["zid"]].any(), (where, k, b)
        if not ref["feasible"][b]:
            assert got["risk"][b] == 0.0 and np.isposinf(got["loss"][b]), (where, b)
            assert not got["grad_logits"][b].any() and not got["grad_cost"][b].any(), (where, b)
            continue
        # sum_i grad_cost[t] = 1 and sum_i grad_logits[t] = 0 for t < I: each of the n allowed
        # classes of the step is within its tolerance, so the sums are within n times it
        ok = R.allowed_classes(c["logits"][b], c["zid"], c["allow_skip"])[:n].sum(axis=1)
        gc = got["grad_cost"][b, :n].astype(np.float64).sum(axis=1)
        gl = got["grad_logits"][b, :n].astype(np.float64).sum(axis=1)
        assert np.all(np.abs(gc - 1.0) <= ok * TOL["grad_cost"]), (where, b)
        assert np.all(np.abs(gl) <= ok * TOL["grad_logits"] * ref["scale"][b]), (where, b)


# ---- 1. accuracy on every case family -----------------------------------------------------------
@pytest.mark.parametrize("D", EC.CLASS_DS)
def test_class_counts(gpu, D):
    name = f"classes-{D}"
    c = _case(name)
    _check(_run(gpu, c, check=True), _ref(name), c, name)


@pytest.mark.parametrize("name", _names("chunk-"))
def test_chunk_edges(gpu, name):
    c = _case(name)
    _check(_run(gpu, c, check=True), _ref(name), c, name)


@pytest.mark.parametrize("name", ["wide", "long-test0", "long-test1", "mode-test0-skip0", "mode-test0-skip1",
                                  "mode-test1-skip0", "mode-test1-skip1"])
def test_wide_window_long_durations_and_modes(gpu, name):
    c = _case(name)
    got = _run(gpu, c, check=True)
    _check(got, _ref(name), c, name)
    assert _ref(name)["feasible"].any()


@pytest.mark.parametrize("name", ["exponent", "cancellation", "constant"])
def test_exponent_range_cancellation_and_constant_cost(gpu, name):
    c = _case(name)
    got = _run(gpu, c, check=True)
    for k in EC.OUTPUTS:
        assert np.isfinite(got[k]).all(), k
    _check(got, _ref(name), c, name)
    if name == "exponent":
        assert np.all(got["loss"] > 80.0 * c["I"])  # far outside the f32 exponent range


@pytest.mark.parametrize("name", EC.VALUE_NAMES)
def test_value_classes(gpu, name):
    # saturated, positive, exponent-heavy and alternating logits (tests/value_cases.py), band and
    # test mode, within the tolerances every other case holds
    c = _case(name)
    got = _run(gpu, c, check=True)
    for k in EC.OUTPUTS:
        assert np.isfinite(got[k]).all(), k
    _check(got, _ref(name), c, name)
    assert _ref(name)["feasible"].all()


# ---- 2. cross-checks against v2_fwd_bwd; the value-only form ------------------------------------
CROSS = (["mode-test0-skip0", "mode-test0-skip1", "mode-test1-skip0", "mode-test1-skip1", "long-test0",
          "long-test1", "wide"] + _names("chunk-"))


@pytest.mark.parametrize("name", CROSS)
def test_loss_and_grad_cost_have_the_bits_of_v2_fwd_bwd(gpu, name):
    c = _case(name)
    got, f4 = _run(gpu, c), _f4(gpu, c)
    assert got["loss"].tobytes() == f4["loss"].tobytes()
    # grad_cost = -grad, bit for bit (zeros: +0 here, +0 there, so compare values)
    assert np.array_equal(got["grad_cost"], -f4["grad"])
    nz = f4["grad"] != 0
    assert got["grad_cost"][nz].tobytes() == (-f4["grad"][nz]).tobytes() and nz.any()


@pytest.mark.parametrize("name", ["classes-3", "classes-17", "classes-64", "wide", "long-test1", "exponent",
                                  "infeasible"] + _names("chunk-"))
def test_value_only_same_bits(gpu, name):
    c = _case(name)
    full, val = _run(gpu, c), _run(gpu, c, need_grad=False)
    assert set(val) == {"risk", "loss", "status"}
    for k in ("risk", "loss"):
        assert val[k].tobytes() == full[k].tobytes(), k


# ---- 3. exact zeros, constant cost, dead edges --------------------------------------------------
@pytest.mark.parametrize("name", ["mode-test0-skip0", "mode-test1-skip1", "classes-33", "wide"])
def test_zero_cost_gives_exact_zeros(gpu, name):
    c = dict(_case(name))
    c["cost"] = np.zeros_like(c["cost"])
    got = _run(gpu, c, check=True)
    assert not got["risk"].view(np.int32).any()          # bitwise +0
    assert not got["grad_logits"].view(np.int32).any()
    assert got["grad_cost"].any()


@pytest.mark.parametrize("name", ["mode-test0-skip1", "mode-test1-skip0", "chunk-4-65"])
def test_constant_cost(gpu, name):
    c = dict(_case(name))
    k = np.float32(2.5)
    c["cost"] = np.full_like(c["cost"], k)
    got = _run(gpu, c, check=True)
    ref = EC.reference(c)
    f = ref["feasible"]
    assert f.any()
    sc = ref["scale"]  # = k * I
    assert np.all(np.abs(got["risk"][f] - k * c["I"][f]) <= TOL["risk"] * sc[f])
    assert np.all(np.abs(got["grad_logits"]).reshape(len(sc), -1).max(axis=1) <= TOL["grad_logits"] * sc)


@pytest.mark.parametrize("name", ["mode-test0-skip0", "mode-test1-skip0", "classes-16"])
def test_costs_of_dead_edges_never_reach_a_result(gpu, name):
    c = dict(_case(name))
    assert not c["allow_skip"]
    lg = c["logits"].copy()
    lg[:, 1::3, 2] = -np.inf     # dead classes beside the zero class
    lg[:, 0, 1] = -np.inf
    c["logits"] = lg
    clean = _run(gpu, c, check=True)
    for bad in (np.nan, np.inf, -np.inf):
        d = dict(c)
        d["cost"] = c["cost"].copy()
        d["cost"][np.isneginf(lg)] = bad
        d["cost"][:, :, c["zid"]] = bad
        got = _run(gpu, d, check=True)
        for k in EC.OUTPUTS:
            assert got[k].tobytes() == clean[k].tobytes(), (k, bad)
    _check(clean, EC.reference(c), c, name + "-dead")


# ---- 4. infeasible rows, error bits -------------------------------------------------------------
def test_infeasible_rows_and_their_neighbours(gpu):
    c = _case("infeasible")
    ref = _ref("infeasible")
    got = _run(gpu, c, check=True)
    _check(got, ref, c, "infeasible")
    assert list(ref["feasible"]) == [True, False, True, False, True, False, False]
    for b in (0, 2, 4):  # a result does not depend on the batch around the utterance
        one = {k: (v[b:b + 1] if k in ("logits", "cost", "I", "O") else v) for k, v in c.items()}
        alone = _run(gpu, one, check=True)
        for k in EC.OUTPUTS:
            assert alone[k][0].tobytes() == got[k][b].tobytes(), (k, b)


def test_bad_length_and_bad_table_status(gpu):
    lib = gpu.load()
    c = dict(_case("infeasible"))
    I2 = c["I"].copy()
    I2[2] = c["logits"].shape[1] + 1  # > max_steps
    d = dict(c, I=I2)
    got = _run(gpu, d)
    assert lib.ssnt_status_from_bits(int(got["status"][0])) == ERR_BAD_LENGTH
    assert got["risk"][2] == 0.0 and np.isposinf(got["loss"][2]) and not got["grad_cost"][2].any()
    clean = _run(gpu, c)
    for k in EC.OUTPUTS:
        assert got[k][0].tobytes() == clean[k][0].tobytes(), k
    with pytest.raises(gpu.SsntError) as e:
        _run(gpu, d, check=True)
    assert e.value.code == ERR_BAD_LENGTH
    d = dict(c, table=np.array([0, 1, -2, 3], np.int32))  # a negative entry: every utterance infeasible
    got = _run(gpu, d)
    assert lib.ssnt_status_from_bits(int(got["status"][0])) == ERR_BAD_INDEX
    assert not got["risk"].any() and np.isposinf(got["loss"]).all()
    assert not got["grad_logits"].any() and not got["grad_cost"].any()
    with pytest.raises(gpu.SsntError) as e:
        _run(gpu, d, check=True)
    assert e.value.code == ERR_BAD_INDEX


# ---- 5. the contract: dead rows and columns, guards, workspace contents -------------------------
@pytest.mark.parametrize("name", ["mode-test0-skip0", "mode-test1-skip1", "long-test1", "chunk-40-33", "infeasible"])
@pytest.mark.parametrize("need_grad", [True, False])
def test_contract(gpu, name, need_grad):
    from test_gpu_contract import three_runs
    lib = gpu.load()
    c = _case(name)
    ref = _ref(name)
    logits, cost, table, I, O = c["logits"], c["cost"], c["table"], c["I"], c["O"]
    B, T, D = logits.shape
    mt, zid, sk, tm = c["mt"], c["zid"], c["allow_skip"], c["test_mode"]
    rng = np.random.default_rng(777)
    other_lg = np.log(rng.dirichlet(np.ones(D), size=(B, T))).astype(np.float32)
    nan1, alt = CC.VALUES["nan_ones"], CC.alternating(B)
    ins = {"A": (logits, cost), "B": (CC.dirty_v2(logits, I, nan1, zid, sk), CC.dirty_v2(cost, I, nan1, zid, sk)),
           "other": (other_lg, cost[::-1].copy()),
           "C": (CC.dirty_v2(logits, I, alt, zid, sk), CC.dirty_v2(cost, I, alt, zid, sk))}
    inputs = {run: {"lg": lg, "cs": cs, "table": table, "il": I, "ol": O} for run, (lg, cs) in ins.items()}
    specs = {"lg": ((B, T, D), F32), "cs": ((B, T, D), F32), "table": ((D,), I32), "il": ((B,), I32),
             "ol": ((B,), I32), "status": ((1,), I32), "risk": ((B,), F32), "loss": ((B,), F32)}
    outs = ["risk", "loss"]
    if need_grad:
        specs["grad_logits"], specs["grad_cost"] = ((B, T, D), F32), ((B, T, D), F32)
        outs += ["grad_logits", "grad_cost"]
    wsb = int(lib.ssnt_v2_expected_cost_workspace_size(B, T, mt, tm, need_grad))
    assert (wsb > 0) == need_grad
    if wsb:
        specs["ws"] = ((wsb,), U8)
    stream = torch.cuda.current_stream().cuda_stream

    def args(v):
        return (v["lg"], v["cs"], v["table"], v["il"], v["ol"], B, T, D, mt, zid, sk, tm, v["risk"], v["loss"],
                v.get("grad_logits"), v.get("grad_cost"), v.get("ws"), wsb, v["status"], stream)

    def check(g, run):
        got = dict(g, status=np.zeros(1, np.int32))
        e = EC.errors(got, ref)
        for k, v in e.items():
            assert v <= TOL[k], (k, v)

    a = three_runs(lib, "ssnt_v2_expected_cost_device", specs, args, inputs, outs, check)
    plain = _run(gpu, c, need_grad=need_grad)
    for k in outs:
        assert a[k].tobytes() == plain[k].tobytes(), k


# ---- 6. every refusal: the return code, the outputs and the status word untouched ---------------
def test_refusals_write_nothing(gpu):
    lib = gpu.load()
    B, T, D, mt = 2, 6, 4, 15
    x = torch.zeros((B, T, D), device=DEV)
    cs = torch.ones((B, T, D), device=DEV)
    tb = torch.arange(D, dtype=I32, device=DEV)
    il = torch.full((B,), T, dtype=I32, device=DEV)
    ol = torch.full((B,), mt, dtype=I32, device=DEV)
    need = int(lib.ssnt_v2_expected_cost_workspace_size(B, T, mt, False, True))
    assert need > 0 and need % 8 == 0
    assert int(lib.ssnt_v2_expected_cost_workspace_size(B, T, mt, False, False)) == 0
    wsbuf = torch.zeros(need + 16, dtype=U8, device=DEV)
    assert wsbuf.data_ptr() % 8 == 0
    ws = wsbuf[:need]
    o = {k: torch.full(s, 7.0, device=DEV) for k, s in (("risk", (B,)), ("loss", (B,)), ("gl", (B, T, D)),
                                                         ("gc", (B, T, D)))}
    st = torch.full((1,), 5, dtype=I32, device=DEV)

    def call(lg=x, c=cs, table=tb, i=il, ol_=ol, b=B, t=T, d=D, m=mt, test=False, risk=o["risk"], loss=o["loss"],
             gl=o["gl"], gc=o["gc"], w=ws, wsb=need):
        return lib.ssnt_v2_expected_cost_device(vp(lg), vp(c), vp(table), vp(i), vp(ol_), b, t, d, m, 0, True, test,
                                                vp(risk), vp(loss), vp(gl), vp(gc), vp(w), wsb, vp(st), None)

    for kw in (dict(lg=None), dict(c=None), dict(table=None), dict(i=None), dict(ol_=None), dict(risk=None),
               dict(b=-1), dict(t=0), dict(d=0), dict(m=-1), dict(m=(1 << 24) + 1)):
        assert call(**kw) == ERR_INVALID_ARG, kw
    assert call(d=65) == ERR_UNSUPPORTED
    assert call(m=1 << 24, test=True) == ERR_UNSUPPORTED  # a row beyond LDS
    assert call(w=None) == ERR_WORKSPACE and call(w=None, wsb=0) == ERR_WORKSPACE
    assert call(wsb=need - 1) == ERR_WORKSPACE
    assert call(w=wsbuf.data_ptr() + 4) == ERR_WORKSPACE  # misaligned
    assert call(gl=None, w=None, wsb=0) == ERR_WORKSPACE    # one gradient still needs the rows
    torch.cuda.synchronize()
    assert all(torch.all(v == 7.0) for v in o.values()) and int(st.item()) == 5
    st.zero_()
    assert call(gl=None, gc=None, w=None, wsb=0) == 0       # value only: the need_grad=false size
    torch.cuda.synchronize()
    assert torch.all(o["gl"] == 7.0) and torch.all(o["gc"] == 7.0)
    val = {k: o[k].clone() for k in ("risk", "loss")}
    assert torch.all(torch.isfinite(val["risk"])) and torch.all(torch.isfinite(val["loss"]))
    assert call(loss=None) == 0 and call(gl=None) == 0 and call(gc=None) == 0 and call() == 0
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    assert torch.equal(o["risk"], val["risk"]) and torch.equal(o["loss"], val["loss"])
    assert torch.allclose(o["gc"].sum(-1), torch.ones((B, T), device=DEV), atol=1e-5)


# ---- 7. determinism, out= reuse ----------------------------------------------------------------
def test_determinism_and_out_reuse(gpu):
    c = _case("classes-17")
    B, T, D = c["logits"].shape
    first = _run(gpu, c)
    out = {"risk": torch.full((B,), 7.0, device=DEV), "loss": torch.full((B,), 7.0, device=DEV),
           "grad_logits": torch.full((B, T, D), 7.0, device=DEV), "grad_cost": torch.full((B, T, D), 7.0, device=DEV),
           "status": torch.ones(1, dtype=I32, device=DEV)}
    args, mode = _args(c)
    for _ in range(3):
        r = gpu.v2_expected_cost(*args, out=out, check=True, **mode)
        for k in out:
            assert r[k].data_ptr() == out[k].data_ptr()
            assert r[k].cpu().numpy().tobytes() == first[k].tobytes(), k
    assert set(first) == {"risk", "loss", "status", "grad_logits", "grad_cost"}
    with pytest.raises(ValueError):
        gpu.v2_expected_cost(*args, out={"risk": torch.empty((B + 1,), device=DEV)}, **mode)
    with pytest.raises(ValueError):
        gpu.v2_expected_cost(*args, out={"grad_logits": torch.empty((B, T, D + 1), device=DEV)}, **mode)
    with pytest.raises(ValueError):
        gpu.v2_expected_cost(*args, out={"grad_cost": torch.empty((B, T, D), dtype=torch.float64, device=DEV)}, **mode)
    with pytest.raises(ValueError):
        gpu.v2_expected_cost(args[0], args[1][:, :, :-1], *args[2:], **mode)


# ---- 8. autograd --------------------------------------------------------------------------------
def test_autograd_of_the_risk(gpu):
    name = "mode-test1-skip1"
    c, ref = _case(name), _ref(name)
    args, mode = _args(c)
    B = len(c["I"])
    wts = torch.tensor([0.5, -1.0, 2.0, 1.5][:B], device=DEV)
    lg = args[0].clone().requires_grad_(True)
    cs = args[1].clone().requires_grad_(True)
    risk = gpu.v2_expected_cost_loss(lg, cs, *args[2:], c["allow_skip"], c["test_mode"], c["mt"])
    (risk * wts).sum().backward()
    w = wts.cpu().numpy().astype(np.float64)
    sc = ref["scale"]
    assert np.max(np.abs(risk.detach().cpu().numpy() - ref["risk"]) / sc) <= TOL["risk"]
    dl = np.abs(lg.grad.cpu().numpy() - ref["grad_logits"] * w[:, None, None]).reshape(B, -1).max(axis=1)
    dc = np.abs(cs.grad.cpu().numpy() - ref["grad_cost"] * w[:, None, None]).reshape(B, -1).max(axis=1)
    assert np.all(dl <= TOL["grad_logits"] * sc * np.abs(w)) and np.all(dc <= TOL["grad_cost"] * np.abs(w))
    # cost alone requiring grad
    cs2 = args[1].clone().requires_grad_(True)
    gpu.v2_expected_cost_loss(args[0], cs2, *args[2:], c["allow_skip"], c["test_mode"], c["mt"]).sum().backward()
    assert np.max(np.abs(cs2.grad.cpu().numpy() - ref["grad_cost"])) <= TOL["grad_cost"]
    # neither: the value-only call, same bits
    plain = gpu.v2_expected_cost_loss(*args, c["allow_skip"], c["test_mode"], c["mt"])
    assert not plain.requires_grad and torch.equal(plain, risk.detach())


@pytest.mark.parametrize("mode_name", ["band", "test_mode", "band-noskip"])
def test_entropy_against_the_brute_force(gpu, mode_name):
    tm, sk = EC.MODES[mode_name]
    logits, _, table, I, O, mt, zid, allow_skip, test_mode = EC.tiny(1, tm, sk)  # (holds -inf logits)
    lg = _t(logits.astype(np.float32)).requires_grad_(True)
    h = gpu.v2_duration_entropy(lg, _t(table, I32), _t(I, I32), _t(O, I32), zid, allow_skip, test_mode, mt)
    hn = h.detach().cpu().numpy()
    href, gref = R.entropy_batch(logits.astype(np.float32), table, I, O, mt, zid, allow_skip, test_mode)
    seen = 0
    for b in range(len(I)):
        bf = R.brute_force(logits[b].astype(np.float32), np.where(np.isfinite(logits[b]), logits[b], 0.0), table,
                           int(I[b]), int(O[b]), mt, zid, allow_skip, test_mode)
        if not bf["feasible"]:
            assert np.isneginf(hn[b])
            continue
        seen += 1
        # H = -loss - risk: the loss within its relative tolerance, the risk within its own
        sc = R.scale(logits[b], logits[b], int(I[b]), zid, allow_skip)
        bound = TOL["loss"] * max(abs(bf["loss"]), 1.0) + TOL["risk"] * sc
        assert abs(hn[b] - bf["entropy"]) <= bound, (b, hn[b], bf["entropy"])
    assert seen >= 1
    feas = np.isfinite(href)
    h[torch.from_numpy(feas).to(DEV)].sum().backward()
    g = lg.grad.cpu().numpy()
    for b in np.nonzero(feas)[0]:
        sc = R.scale(logits[b], logits[b], int(I[b]), zid, allow_skip)
        # dH = posterior - (grad_logits + grad_cost): three terms, each within its tolerance
        assert np.max(np.abs(g[b] - gref[b])) <= TOL["grad_logits"] * sc + 2 * TOL["grad_cost"], b


def test_entropy_gradient_at_a_larger_case(gpu):
    c = _case("chunk-40-33")
    lgn = c["logits"]
    lg = _t(lgn).requires_grad_(True)
    h = gpu.v2_duration_entropy(lg, _t(c["table"], I32), _t(c["I"], I32), _t(c["O"], I32), c["zid"],
                                c["allow_skip"], c["test_mode"], c["mt"])
    href, gref = R.entropy_batch(lgn, c["table"], c["I"], c["O"], c["mt"], c["zid"], c["allow_skip"], c["test_mode"])
    assert np.isfinite(href).all()
    ref = EC.reference(dict(c, cost=lgn))
    sc = ref["scale"]
    hn = h.detach().cpu().numpy()
    assert np.all(np.abs(hn - href) <= TOL["loss"] * np.maximum(np.abs(ref["loss"]), 1.0) + TOL["risk"] * sc)
    h.sum().backward()
    d = np.abs(lg.grad.cpu().numpy() - gref).reshape(len(sc), -1).max(axis=1)
    assert np.all(d <= TOL["grad_logits"] * sc + 2 * TOL["grad_cost"])
