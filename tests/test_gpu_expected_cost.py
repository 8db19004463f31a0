"""ssnt_expected_cost on the GPU against the float64 reference (tests/expected_cost_ref.py,
DESIGN.md 2.8): lane slices, chunk edges, modes, the value-only form, infeasible rows, exponent
range, cancellation, exact zeros, cross-checks against ssnt_fwd_bwd, the contract (dead cells,
guards, refused calls), determinism and autograd. Errors are normalised as
tests/expected_cost_cases.py `errors` does; the tolerances are 4x the worst value
tools/bench_expected_cost.py --accuracy measured (profiles/expected_cost_accuracy.jsonl, line
"worst"), rounded up to one significant digit."""
import functools

import numpy as np
import pytest
import torch

import contract_cases as CC
import expected_cost_cases as EC
import expected_cost_ref as R
import guarded as G
from gpu_util import DEV, _t

pytestmark = pytest.mark.gpu

F32, I32, U8 = torch.float32, torch.int32, torch.uint8
BAD_LENGTH_BIT = 4
ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = 1, 5, 6

# 4x profiles/expected_cost_accuracy.jsonl line "worst", one significant digit, rounded up
TOL = {
    "risk": 4e-7,        # worst.errors.risk 9.38e-8 (large-B64-T2000-U400-entropy)
    "loss": 3e-6,        # worst.errors.loss 5.46e-7 (chunk-130-1: relative, at a loss below 1)
    "grad_trans": 7e-7,  # worst.errors.grad_trans 1.52e-7 (large-B64-T2000-U400-entropy)
    "grad_cost": 8e-6,   # worst.errors.grad_cost 1.90e-6 (lane-1024)
    "grad_obs": 3e-7,    # worst.errors.grad_obs 7.49e-8 (lane-1)
}
# ssnt_fwd_bwd against float64 (5.6e-6 relative on alpha at the largest BASELINE
# shape; the shapes here are far smaller), for the cross-checks that compare two f32 results
FWD_BWD_TOL = 5.6e-6


def _run(gpu, c, need_grad=True, out=None, check=False):
    r = gpu.ssnt_expected_cost(_t(c["lt"]), _t(c["cost"]), _t(c["S"]), _t(c["P"]), _t(c["lo"]),
                               terminal_emit=c["terminal"], need_grad=need_grad, check=check, out=out)
    return {k: v.cpu().numpy() for k, v in r.items()}


@functools.lru_cache(maxsize=None)
def _makers():
    import ssnt_tts_amd
    ab = ssnt_tts_amd.load_ab()  # (a host query: no GPU call)
    return EC.case_makers(lambda U, obs: ab.ssnt_expected_cost_chunk_rows(U, int(obs)))


@functools.lru_cache(maxsize=None)
def _case(name):
    return _makers()[name]()


@functools.lru_cache(maxsize=None)
def _ref(name):
    return EC.reference(_case(name))


def _check(got, ref, c, where=""):
    """Every output within tolerance, the exact parts exact, and the two identities per step."""
    e = EC.errors(got, ref)
    print(where, e)
    for k, v in e.items():
        assert v <= TOL[k], (where, k, v, TOL[k])
    assert int(got["status"][0]) == 0
    B, T, U = c["lt"].shape[:3]
    for b in range(B):
        S, P = int(c["S"][b]), int(c["P"][b])
        live = R.live_edges((T, U), S, P, c["terminal"])
        for k in ("grad_trans", "grad_cost"):
            assert not got[k][b][~live].any(), (where, k, b)  # exact 0 outside the lattice
        if "grad_obs" in got:
            cells = np.zeros((T, U), bool)
            cells[:max(S - 1, 0), :P] = True
            assert not got["grad_obs"][b][~cells].any(), (where, b)
        if not ref["feasible"][b]:
            continue
        if c["terminal"]:
            assert got["grad_cost"][b, S - 1, P - 1, 0] == 1.0 and got["grad_trans"][b, S - 1, P - 1, 0] == 0.0
        # sum_{p,k} grad_cost[s] = 1 and sum_{p,k} grad_trans[s] = 0 for s < S-1: each of the n live
        # edges of the step is within its tolerance, so the sums are within n times it
        n = live[:S - 1].sum(axis=(1, 2))
        gc = got["grad_cost"][b, :S - 1].astype(np.float64).sum(axis=(1, 2))
        gt = got["grad_trans"][b, :S - 1].astype(np.float64).sum(axis=(1, 2))
        assert np.all(np.abs(gc - 1.0) <= n * TOL["grad_cost"]), (where, b)
        assert np.all(np.abs(gt) <= n * TOL["grad_trans"] * ref["scale"][b]), (where, b)


@pytest.mark.parametrize("U", EC.LANE_US)
def test_lane_slices(gpu, U):
    name = f"lane-{U}"
    c = _case(name)
    _check(_run(gpu, c), _ref(name), c, name)


def _chunk_names():
    # (collected without a GPU too: the names come from the cases only when the library is there)
    try:
        return [n for n in _makers() if n.startswith("chunk-")]
    except Exception:  # noqa: BLE001
        return ["chunk-unavailable"]


@pytest.mark.parametrize("name", _chunk_names())
def test_chunks(gpu, name):
    c = _case(name)
    _check(_run(gpu, c), _ref(name), c, name)


@pytest.mark.parametrize("terminal", [False, True])
@pytest.mark.parametrize("obs", [False, True])
def test_modes(gpu, obs, terminal):
    name = f"mode-obs{int(obs)}-term{int(terminal)}"
    c = _case(name)
    _check(_run(gpu, c), _ref(name), c, name)


@pytest.mark.parametrize("name", ["exponent", "cancellation"])
def test_exponent_range_and_cancellation(gpu, name):
    c = _case(name)
    got = _run(gpu, c)
    for k in EC.OUTPUTS:
        if k in got:
            assert np.isfinite(got[k]).all(), k
    _check(got, _ref(name), c, name)


@pytest.mark.parametrize("name", EC.VALUE_NAMES)
def test_value_classes(gpu, name):
    # saturated, positive, exponent-heavy and alternating log_trans (tests/value_cases.py) within
    # the tolerances every other case holds
    c = _case(name)
    got = _run(gpu, c)
    for k in EC.OUTPUTS:
        if k in got:
            assert np.isfinite(got[k]).all(), k
    _check(got, _ref(name), c, name)


@pytest.mark.parametrize("name", ["lane-65", "lane-513", "mode-obs1-term1", "mode-obs0-term0", "exponent",
                                  "chunk-5-3", "chunk-130-2"])
def test_value_only_same_bits(gpu, name):
    c = _case(name)
    full, val = _run(gpu, c), _run(gpu, c, need_grad=False)
    assert set(val) == {"risk", "loss", "status"}
    assert CC.same_bits(val["risk"], full["risk"]) and CC.same_bits(val["loss"], full["loss"])


def test_value_only_chunk_edges(gpu):
    """Every T around the chunk edges: the value-only form's bits are the full call's."""
    for name in _chunk_names():
        c = _case(name)
        full, val = _run(gpu, c), _run(gpu, c, need_grad=False)
        assert CC.same_bits(val["risk"], full["risk"]) and CC.same_bits(val["loss"], full["loss"]), name


def _infeasible_case():
    c = EC.make(6, 8, 5, 99, obs=True, S=[8, 2, 0, 4, 6, 7], P=[5, 3, 2, 0, 3, 4])
    c["lt"][4, 2, :, 1] = -np.inf   # utterance 4: a row of -inf shifts ...
    c["lt"][4, :, 1, 1] = -np.inf   # ... and none out of position 1 at any step: P - 1 is out of reach, Z = 0
    return c


def test_infeasible_rows(gpu):
    c = _infeasible_case()
    ref = EC.reference(c)
    assert list(ref["feasible"]) == [True, False, False, False, False, True]
    got = _run(gpu, c)
    _check(got, ref, c, "infeasible")
    for b in (1, 2, 3, 4):
        assert got["risk"][b] == 0.0 and np.isposinf(got["loss"][b])
        assert not got["grad_trans"][b].any() and not got["grad_cost"][b].any() and not got["grad_obs"][b].any()
    # the neighbours are what they are alone
    for b in (0, 5):
        one = {k: (v[b:b + 1] if isinstance(v, np.ndarray) else v) for k, v in c.items()}
        alone = _run(gpu, one)
        for k in EC.OUTPUTS:
            assert CC.same_bits(alone[k][0], got[k][b]), (k, b)


def test_bad_length(gpu):
    c = EC.make(3, 6, 4, 3, obs=False, S=[6, 7, 5], P=[4, 3, 5])
    got = _run(gpu, c)
    assert int(got["status"][0]) == BAD_LENGTH_BIT
    for b in (1, 2):
        assert got["risk"][b] == 0.0 and np.isposinf(got["loss"][b]) and not got["grad_cost"][b].any()
    assert np.isfinite(got["loss"][0]) and got["grad_cost"][0].any()
    with pytest.raises(gpu.SsntError):
        _run(gpu, c, check=True)


def test_exact_zeros(gpu):
    for name in ("lane-65", "mode-obs1-term1", "chunk-130-3"):
        c = dict(_case(name))
        c["cost"] = np.zeros_like(c["cost"])
        got = _run(gpu, c)
        assert not got["risk"].any() and not got["grad_trans"].any(), name
        if "grad_obs" in got:
            assert not got["grad_obs"].any(), name
        assert got["grad_cost"].any()


def test_constant_cost(gpu):
    c = dict(_case("lane-129"))
    c["cost"] = np.full_like(c["cost"], 2.5)
    _check(_run(gpu, c), EC.reference(c), c, "constant")


@pytest.mark.parametrize("name", ["lane-64", "lane-257", "mode-obs1-term1", "mode-obs1-term0"])
def test_cross_checks_against_fwd_bwd(gpu, name):
    c = _case(name)
    got = _run(gpu, c)
    fb = gpu.ssnt_fwd_bwd(_t(c["lt"]), _t(c["S"]), _t(c["P"]), _t(c["lo"]), terminal_emit=c["terminal"])
    g, loss = fb["grad"].cpu().numpy().astype(np.float64), fb["loss"].cpu().numpy().astype(np.float64)
    # two f32 results, each within its own tolerance of the float64 value
    assert np.abs(got["grad_cost"] + g).max() <= TOL["grad_cost"] + FWD_BWD_TOL
    fin = np.isfinite(loss)
    assert np.array_equal(fin, np.isfinite(got["loss"]))
    den = np.maximum(np.abs(loss[fin]), 1.0)
    assert np.all(np.abs(got["loss"][fin] - loss[fin]) / den <= TOL["loss"] + FWD_BWD_TOL)


# ---- the contract: dead cells, guards, workspace contents, refused calls --------------------------
def _specs(c, wsb, ws_offset=0):
    B, T, U = c["lt"].shape[:3]
    specs = {"lt": ((B, T, U, 2), F32), "cost": ((B, T, U, 2), F32), "sl": ((B,), I32), "pl": ((B,), I32),
             "status": ((1,), I32), "risk": ((B,), F32), "loss": ((B,), F32),
             "grad_trans": ((B, T, U, 2), F32), "grad_cost": ((B, T, U, 2), F32)}
    if c["lo"] is not None:
        specs["lo"] = ((B, T, U), F32)
        specs["grad_obs"] = ((B, T, U), F32)
    if wsb:
        specs["ws"] = ((wsb,), U8, ws_offset)
    return specs


def _args(c, wsb, flags=None):
    B, T, U = c["lt"].shape[:3]
    flags = int(c["terminal"]) if flags is None else flags
    stream = torch.cuda.current_stream().cuda_stream

    def args(v, U=U, wsb=wsb):
        return (v["lt"], v.get("lo"), v["cost"], v["sl"], v["pl"], B, T, U, flags, v["risk"], v["loss"],
                v["grad_trans"], v["grad_cost"], v.get("grad_obs"), v.get("ws"), wsb, v["status"], stream)
    return args


def _dirty(c, value):
    lt, lo = CC.dirty_lattice(c["lt"], c["lo"], c["S"], c["P"], value, c["terminal"])
    cost, _ = CC.dirty_lattice(c["cost"], None, c["S"], c["P"], value, c["terminal"])
    return lt, lo, cost


@pytest.mark.parametrize("name", ["lane-65", "lane-129", "lane-513", "mode-obs1-term0", "chunk-130-3"])
def test_contract(gpu, name):
    """Runs A / B / C of tests/test_gpu_contract.py: dead cells of log_trans, log_obs and cost dirty,
    guards around every tensor, the workspace (8-byte aligned only) zeroed, 0xFF and stale."""
    from test_gpu_contract import three_runs
    lib = gpu.load()
    c = _case(name)
    ref = _ref(name)
    B, T, U = c["lt"].shape[:3]
    other = EC.make(B, T, U, 4242, obs=c["lo"] is not None)
    ins = {"A": (c["lt"], c["lo"], c["cost"]), "B": _dirty(c, CC.VALUES["nan_ones"]),
           "other": (other["lt"], other["lo"], other["cost"]), "C": _dirty(c, CC.alternating(B))}
    inputs = {}
    for run, (lt, lo, cost) in ins.items():
        inputs[run] = {"lt": lt, "cost": cost, "sl": c["S"], "pl": c["P"]}
        if lo is not None:
            inputs[run]["lo"] = lo
    wsb = int(lib.ssnt_expected_cost_workspace_size(B, T, U))
    assert wsb > 0
    outs = [k for k in EC.OUTPUTS if k != "grad_obs" or c["lo"] is not None]

    def check(got, run):
        _check(dict(got, status=np.zeros(1, np.int32)), ref, c, f"{name} run {run}")

    three_runs(lib, "ssnt_expected_cost_device", _specs(c, wsb, ws_offset=8), _args(c, wsb), inputs, outs, check)


def test_workspace_contents_do_not_matter(gpu):
    lib = gpu.load()
    c = _case("lane-129")
    B, T, U = c["lt"].shape[:3]
    wsb = int(lib.ssnt_expected_cost_workspace_size(B, T, U))
    arena, v = G.lay_out(DEV, _specs(c, wsb))
    for k, a in (("lt", c["lt"]), ("cost", c["cost"]), ("sl", c["S"]), ("pl", c["P"]), ("lo", c["lo"])):
        G.put(v[k], a)
    outs = {}
    for fill in (0xA5, 0xFF, None):  # 0xFF: every f32 of it is a NaN; None: what the last run left
        if fill is not None:
            G.fill_bytes(v["ws"], fill)
        v["status"].zero_()
        assert G.call(lib, "ssnt_expected_cost_device", *_args(c, wsb)(v)) == 0
        torch.cuda.synchronize()
        arena.check()
        outs[fill] = {k: G.get(v[k]) for k in EC.OUTPUTS}
    assert CC.same_bits(outs[0xA5], outs[0xFF]) and CC.same_bits(outs[0xA5], outs[None])


def test_refused_calls_write_nothing(gpu):
    lib = gpu.load()
    c = _case("mode-obs1-term1")
    B, T, U = c["lt"].shape[:3]
    wsb = int(lib.ssnt_expected_cost_workspace_size(B, T, U))
    arena, v = G.lay_out(DEV, _specs(c, wsb))
    for k, a in (("lt", c["lt"]), ("cost", c["cost"]), ("sl", c["S"]), ("pl", c["P"]), ("lo", c["lo"])):
        G.put(v[k], a)
    written = list(EC.OUTPUTS) + ["ws", "status"]
    for k in written:
        G.fill_bytes(v[k], 0x5A)
    before = {k: G.get(v[k]) for k in written}
    ok = _args(c, wsb)(v)
    too_wide = list(ok)
    too_wide[7] = 1025
    short = list(ok)
    short[15] = wsb - 1
    no_ws = list(ok)
    no_ws[14] = None
    misaligned = list(ok)
    misaligned[14] = v["ws"].data_ptr() + 4
    bad_flag = list(ok)
    bad_flag[8] = 2  # SSNT_FLAG_ZERO_INFINITY is not accepted here
    no_obs = list(ok)
    no_obs[1] = None  # grad_obs without log_obs
    for args, code in ((too_wide, ERR_UNSUPPORTED), (short, ERR_WORKSPACE), (no_ws, ERR_WORKSPACE),
                       (misaligned, ERR_WORKSPACE), (bad_flag, ERR_INVALID_ARG), (no_obs, ERR_INVALID_ARG)):
        assert G.call(lib, "ssnt_expected_cost_device", *args) == code
    torch.cuda.synchronize()
    arena.check()
    for k in written:
        assert CC.same_bits(G.get(v[k]), before[k]), k
    assert lib.ssnt_expected_cost_workspace_size(B, T, 1025) == 0
    # value only: no workspace at all
    val = list(ok)
    val[11] = val[12] = val[13] = val[14] = None
    val[15] = 0
    v["status"].zero_()
    assert G.call(lib, "ssnt_expected_cost_device", *val) == 0
    torch.cuda.synchronize()
    arena.check()
    ref = _ref("mode-obs1-term1")
    assert np.abs(G.get(v["risk"]) - ref["risk"]).max() <= TOL["risk"] * ref["scale"].max()


def test_deterministic_and_out_reuse(gpu):
    c = _case("lane-257")
    a, b = _run(gpu, c), _run(gpu, c)
    assert CC.same_bits(a, b)
    B, T, U = c["lt"].shape[:3]
    out = {"risk": torch.full((B,), 7.0, device=DEV), "loss": torch.full((B,), 7.0, device=DEV),
           "grad_trans": torch.full((B, T, U, 2), 7.0, device=DEV),
           "grad_cost": torch.full((B, T, U, 2), 7.0, device=DEV),
           "grad_obs": torch.full((B, T, U), 7.0, device=DEV),
           "status": torch.ones(1, dtype=torch.int32, device=DEV)}
    for _ in range(2):
        r = _run(gpu, c, out=out)
        assert CC.same_bits(r, a)
    assert CC.same_bits(out["grad_trans"].cpu().numpy(), a["grad_trans"])
    with pytest.raises(ValueError):
        _run(gpu, c, out={"risk": torch.empty(B + 1, device=DEV)})


# ---- autograd -------------------------------------------------------------------------------------
def _autograd_case(obs):
    return EC.make(3, 9, 4, 17, obs, S=[9, 6, 4], P=[4, 3, 4])


@pytest.mark.parametrize("obs", [False, True])
def test_autograd_expected_cost_loss(gpu, obs):
    c = _autograd_case(obs)
    ref = EC.reference(c)
    lt, cost = _t(c["lt"]).requires_grad_(), _t(c["cost"]).requires_grad_()
    lo = _t(c["lo"]).requires_grad_() if obs else None
    w = torch.tensor([1.0, -2.0, 0.5], device=DEV)
    risk = gpu.ssnt_expected_cost_loss(lt, cost, _t(c["S"]), _t(c["P"]), lo)
    assert np.abs(risk.detach().cpu().numpy() - ref["risk"]).max() <= TOL["risk"] * ref["scale"].max()
    (risk * w).sum().backward()
    wn = w.cpu().numpy().astype(np.float64)
    sc = ref["scale"]
    for t, k, s in ((lt, "grad_trans", sc), (cost, "grad_cost", np.ones(3))) + (((lo, "grad_obs", sc),) if obs else ()):
        want = ref[k] * wn.reshape((3,) + (1,) * (ref[k].ndim - 1))
        err = np.abs(t.grad.cpu().numpy() - want).reshape(3, -1).max(axis=1)
        assert np.all(err <= TOL[k] * s * np.abs(wn)), (k, err)
    # cost alone: log_trans gets no gradient
    lt2, cost2 = _t(c["lt"]), _t(c["cost"]).requires_grad_()
    gpu.ssnt_expected_cost_loss(lt2, cost2, _t(c["S"]), _t(c["P"]), _t(c["lo"])).sum().backward()
    assert np.abs(cost2.grad.cpu().numpy() - ref["grad_cost"]).max() <= TOL["grad_cost"]


@pytest.mark.parametrize("terminal", [False, True])
@pytest.mark.parametrize("obs", [False, True])
def test_autograd_alignment_entropy(gpu, obs, terminal):
    """H = -loss - risk(entropy cost) (- log_obs[0,0]); d H / d log_trans = -grad_trans and
    d H / d log_obs = -grad_obs of the reference at the entropy cost (the posterior terms of
    -d loss and of d risk / d cost cancel)."""
    c = _autograd_case(obs)
    c["terminal"] = terminal
    B = 3
    c["cost"] = np.stack([R.entropy_cost(c["lt"][b], int(c["S"][b]), c["lo"][b] if obs else None)
                          for b in range(B)]).astype(np.float32)
    ref = EC.reference(c)
    lt = _t(c["lt"]).requires_grad_()
    lo = _t(c["lo"]).requires_grad_() if obs else None
    h = gpu.ssnt_alignment_entropy(lt, _t(c["S"]), _t(c["P"]), lo, terminal)
    want = -ref["loss"] - ref["risk"] - (c["lo"][:, 0, 0].astype(np.float64) if obs else 0.0)
    # ln Z within its relative tolerance (ours and ssnt_fwd_bwd's), risk within its own
    tol_h = (TOL["loss"] + FWD_BWD_TOL) * np.abs(ref["loss"]) + TOL["risk"] * ref["scale"] + 1e-6
    assert np.all(np.abs(h.detach().cpu().numpy() - want) <= tol_h), (h, want)
    h.sum().backward()
    # d H / d lt = (q_fwd_bwd - q_ours) - grad_trans: two edge posteriors and one covariance
    tol_g = (TOL["grad_cost"] + FWD_BWD_TOL) + TOL["grad_trans"] * ref["scale"]
    err = np.abs(lt.grad.cpu().numpy() + ref["grad_trans"]).reshape(B, -1).max(axis=1)
    assert np.all(err <= tol_g), err
    if obs:
        err = np.abs(lo.grad.cpu().numpy() + ref["grad_obs"]).reshape(B, -1).max(axis=1)
        assert np.all(err <= 2 * (TOL["grad_cost"] + FWD_BWD_TOL) + TOL["grad_obs"] * ref["scale"]), err
