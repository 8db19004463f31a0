"""ssnt_duration_posterior on the GPU against the float64 reference
(tests/duration_posterior_ref.py): lane slices, chunk and tile edges, bin edges, the
three tail regimes, modes, degenerate lattices, exponent range, value classes, one larger shape, the
single-path lattice, the identities (exact zeros, row sums, mean duration, loss bits), the contract
(dead cells, guards, workspace and output contents, alone against batch, refused calls) and
determinism. dur_post errors are absolute (a probability), the loss error relative, as
tests/duration_posterior_cases.py `errors` has them; the tolerances are 4x the worst value
tools/bench_duration_posterior.py --accuracy measured (profiles/duration_posterior_accuracy.jsonl,
line "worst"), rounded up to one significant digit."""
import functools

import numpy as np
import pytest
import torch

import contract_cases as CC
import duration_posterior_cases as DC
import guarded as G
from gpu_util import DEV, _t

pytestmark = pytest.mark.gpu

F32, I32, U8 = torch.float32, torch.int32, torch.uint8
BAD_LENGTH_BIT = 4
ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = 1, 5, 6

# 4x profiles/duration_posterior_accuracy.jsonl line "worst", one significant digit, rounded up
TOL = {
    "dur_post": 8e-6,  # worst.errors.dur_post 1.98e-6 (lane-1024)
    "loss": 2e-5,      # worst.errors.loss 3.63e-6 (chunk-1: relative, at a loss of 0.0059)
}
# tests/test_gpu_expected_cost.py TOL["grad_cost"]: the edge posterior of ssnt_expected_cost
# against float64, for the mean-duration identity, which compares two f32 results
GRAD_COST_TOL = 8e-6


def _run(gpu, c, out=None, check=False, D=None):
    r = gpu.ssnt_duration_posterior(_t(c["lt"]), _t(c["S"]), _t(c["P"]), c["D"] if D is None else D,
                                    _t(c["lo"]), terminal_emit=c["terminal"], out=out, check=check)
    return {k: v.cpu().numpy() for k, v in r.items()}


@functools.lru_cache(maxsize=None)
def _block():
    import ssnt_tts_amd
    blk = ssnt_tts_amd.load_ab().ssnt_duration_posterior_block(64, 32, 0)  # (a host query: no GPU call)
    return blk & 0xFFFF, blk >> 16


@functools.lru_cache(maxsize=None)
def _makers():
    import ssnt_tts_amd
    ab = ssnt_tts_amd.load_ab()
    return DC.case_makers(*_block(), lambda U, obs: ab.ssnt_duration_posterior_sweep_rows(U, int(obs)))


@functools.lru_cache(maxsize=None)
def _case(name):
    return _makers()[name]()


@functools.lru_cache(maxsize=None)
def _ref(name):
    return DC.reference(_case(name))


def _zero_bits(a):
    return not np.ascontiguousarray(a).view(np.uint32).any()


def _check(gpu, got, ref, c, where="", identities=True):
    """Both outputs within tolerance, the exact zeros bitwise, and the identities."""
    e = DC.errors(got, ref)
    print(where, e)
    for k, v in e.items():
        assert v <= TOL[k], (where, k, v, TOL[k])
    assert int(got["status"][0]) == 0
    dp = got["dur_post"]
    D = c["D"]
    assert dp.shape == ref["dur_post"].shape and np.isfinite(dp).all()
    assert _zero_bits(dp[DC.impossible(c)]), where  # bin 0, rows p >= P, bins no position can fill
    B = len(c["S"])
    for b in range(B):
        P = int(c["P"][b])
        if not ref["feasible"][b]:
            assert _zero_bits(dp[b]) and np.isposinf(got["loss"][b]), (where, b)
            continue
        # each of the D bins is within its tolerance, so a row's sum is within D times it
        assert np.abs(dp[b, :P].astype(np.float64).sum(axis=1) - 1.0).max() <= D * TOL["dur_post"], (where, b)
    if not identities:
        return
    ec = gpu.ssnt_expected_cost(_t(c["lt"]), torch.zeros(c["lt"].shape, device=DEV), _t(c["S"]), _t(c["P"]),
                                _t(c["lo"]), terminal_emit=c["terminal"], need_grad=True)
    val = gpu.ssnt_expected_cost(_t(c["lt"]), torch.zeros(c["lt"].shape, device=DEV), _t(c["S"]), _t(c["P"]),
                                 _t(c["lo"]), terminal_emit=c["terminal"], need_grad=False)
    assert CC.same_bits(got["loss"], val["loss"].cpu().numpy()), where
    gc = ec["grad_cost"].cpu().numpy().astype(np.float64)
    for b in range(B):
        S, P = int(c["S"][b]), int(c["P"][b])
        L = S - P + 1
        if not ref["feasible"][b] or D - 1 < L:
            continue  # (a true tail: the last bin is no duration)
        # the mean duration = the occupancy: the posterior of entering (s, p) by either edge, plus
        # the start cell. L bins weighted d <= L, each within TOL; 2 (S-1) edge posteriors, each
        # within ssnt_expected_cost's tolerance
        occ = gc[b, :S - 1, :P, 0].sum(axis=0)
        occ[1:] += gc[b, :S - 1, :P - 1, 1].sum(axis=0)
        occ[0] += 1.0
        mean = (dp[b, :P].astype(np.float64) * np.arange(D)).sum(axis=1)
        bound = TOL["dur_post"] * L * (L + 1) / 2 + GRAD_COST_TOL * 2 * max(S - 1, 1)
        assert np.abs(mean - occ).max() <= bound, (where, b, np.abs(mean - occ).max(), bound)


def _names(prefix):
    # (collected without a GPU too: the names come from the cases only when the library is there)
    try:
        return [n for n in _makers() if n.startswith(prefix)]
    except Exception:  # noqa: BLE001
        return [prefix + "unavailable"]


@pytest.mark.parametrize("U", DC.LANE_US)
def test_lane_slices(gpu, U):
    name = f"lane-{U}"
    c = _case(name)
    _check(gpu, _run(gpu, c), _ref(name), c, name)


@pytest.mark.parametrize("name", _names("chunk-"))
def test_chunk_and_tile_edges(gpu, name):
    c = _case(name)
    _check(gpu, _run(gpu, c), _ref(name), c, name)


@pytest.mark.parametrize("name", _names("sweep-"))
def test_sweep_chunk_edges(gpu, name):
    # the sweeps stage no cost, so their chunks are deeper than ssnt_expected_cost's
    c = _case(name)
    _check(gpu, _run(gpu, c), _ref(name), c, name)


@pytest.mark.parametrize("D", DC.BIN_DS_SHORT + DC.BIN_DS_LONG)
def test_bin_edges(gpu, D):
    name = f"bins-{D}"
    c = _case(name)
    got = _run(gpu, c)
    _check(gpu, got, _ref(name), c, name)
    if D == 2:  # the tail alone: every live row is (0, 1)
        for b in range(len(c["S"])):
            P = int(c["P"][b])
            assert _zero_bits(got["dur_post"][b, :, 0])
            assert np.abs(got["dur_post"][b, :P, 1] - 1.0).max() <= TOL["dur_post"]


@pytest.mark.parametrize("D", DC.TAIL_DS)
def test_tail_regimes(gpu, D):
    name = f"tail-{D}"
    c = _case(name)
    got = _run(gpu, c)
    _check(gpu, got, _ref(name), c, name)
    L = int(c["S"][0]) - int(c["P"][0]) + 1
    P = int(c["P"][0])
    if D - 1 < L:
        assert (got["dur_post"][0, :P, D - 1] > 0).all()  # a true tail holds mass
    elif D - 1 > L:
        assert _zero_bits(got["dur_post"][0, :, L + 1:])  # no bin beyond L, and no tail


@pytest.mark.parametrize("terminal", [False, True])
@pytest.mark.parametrize("obs", [False, True])
def test_modes(gpu, obs, terminal):
    name = f"mode-obs{int(obs)}-term{int(terminal)}"
    c = _case(name)
    _check(gpu, _run(gpu, c), _ref(name), c, name)


@pytest.mark.parametrize("D", DC.DEGENERATE_DS)
def test_degenerate_lattices(gpu, D):
    name = f"degenerate-{D}"
    c = _case(name)
    got = _run(gpu, c)
    _check(gpu, got, _ref(name), c, name)
    dp = got["dur_post"]
    for b in (0, 1):  # S = P: every duration is 1, and nothing else holds a bit
        P = int(c["P"][b])
        assert np.abs(dp[b, :P, 1] - 1.0).max() <= TOL["dur_post"]
        assert _zero_bits(dp[b, :, 2:])
    S = int(c["S"][2])  # P = 1: one position holds all S steps
    assert abs(dp[2, 0, min(S, D - 1)] - 1.0) <= TOL["dur_post"]
    assert _zero_bits(np.delete(dp[2, 0], min(S, D - 1)))


def test_exponent_range(gpu):
    c = _case("exponent")
    _check(gpu, _run(gpu, c), _ref("exponent"), c, "exponent")


@pytest.mark.parametrize("name", DC.EC.VALUE_NAMES)
def test_value_classes(gpu, name):
    c = _case(name)
    _check(gpu, _run(gpu, c), _ref(name), c, name)


def test_larger_shape(gpu):
    c = _case("larger")
    _check(gpu, _run(gpu, c), _ref("larger"), c, "larger")


@pytest.mark.parametrize("obs", [False, True])
def test_single_path(gpu, obs):
    name = "single-path-obs" if obs else "single-path"
    c, dur = DC.single_path(obs)
    got = _run(gpu, c)
    _check(gpu, got, _ref(name), c, name)
    vit = gpu.ssnt_viterbi_align(_t(c["lt"]), _t(c["S"]), _t(c["P"]), _t(c["lo"]), terminal_emit=c["terminal"])
    vdur = vit["duration"].cpu().numpy()
    assert np.array_equal(vdur, dur)
    B, U, D = got["dur_post"].shape
    hot = np.zeros((B, U, D), bool)
    for b in range(B):
        for p in range(int(c["P"][b])):
            hot[b, p, min(int(vdur[b, p]), D - 1)] = True
    assert np.abs(got["dur_post"][hot] - 1.0).max() <= TOL["dur_post"]
    assert _zero_bits(got["dur_post"][~hot])


# ---- infeasible rows, bad lengths -----------------------------------------------------------------
def _infeasible_case():
    c = DC.make(6, 8, 5, 6, 99, obs=True, S=[8, 2, 0, 4, 6, 7], P=[5, 3, 2, 0, 3, 4])
    c["lt"][4, 2, :, 1] = -np.inf   # utterance 4: a row of -inf shifts ...
    c["lt"][4, :, 1, 1] = -np.inf   # ... and none out of position 1 at any step: P - 1 is out of reach, Z = 0
    return c


def _alone(c, b, crop=False):
    """Utterance b as a batch of one; crop: in tensors no larger than its own lattice."""
    S, P = (int(c["S"][b]), int(c["P"][b])) if crop else c["lt"].shape[1:3]
    one = {k: (v[b:b + 1] if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    one["lt"] = np.ascontiguousarray(one["lt"][:, :S, :P])
    if one["lo"] is not None:
        one["lo"] = np.ascontiguousarray(one["lo"][:, :S, :P])
    return one


def test_infeasible_rows(gpu):
    c = _infeasible_case()
    ref = DC.reference(c)
    assert list(ref["feasible"]) == [True, False, False, False, False, True]
    got = _run(gpu, c)
    _check(gpu, got, ref, c, "infeasible")
    for b in (0, 5):  # the neighbours are what they are alone
        alone = _run(gpu, _alone(c, b))
        for k in DC.OUTPUTS:
            assert CC.same_bits(alone[k][0], got[k][b]), (k, b)


def test_bad_length(gpu):
    c = DC.make(3, 6, 4, 5, 3, obs=False, S=[6, 7, 5], P=[4, 3, 5])
    got = _run(gpu, c)
    assert int(got["status"][0]) == BAD_LENGTH_BIT
    for b in (1, 2):
        assert np.isposinf(got["loss"][b]) and _zero_bits(got["dur_post"][b])
    assert np.isfinite(got["loss"][0]) and got["dur_post"][0].any()
    with pytest.raises(gpu.SsntError):
        _run(gpu, c, check=True)


# ---- the contract: dead cells, guards, workspace and output contents, refused calls --------------
def _specs(c, wsb, ws_offset=0):
    B, T, U = c["lt"].shape[:3]
    specs = {"lt": ((B, T, U, 2), F32), "sl": ((B,), I32), "pl": ((B,), I32), "status": ((1,), I32),
             "dur_post": ((B, U, c["D"]), F32), "loss": ((B,), F32)}
    if c["lo"] is not None:
        specs["lo"] = ((B, T, U), F32)
    specs["ws"] = ((wsb,), U8, ws_offset)
    return specs


def _args(c, wsb, flags=None):
    B, T, U = c["lt"].shape[:3]
    flags = int(c["terminal"]) if flags is None else flags
    stream = torch.cuda.current_stream().cuda_stream

    def args(v):
        return (v["lt"], v.get("lo"), v["sl"], v["pl"], B, T, U, c["D"], flags, v["dur_post"], v["loss"],
                v["ws"], wsb, v["status"], stream)
    return args


@pytest.mark.parametrize("name", ["lane-65", "lane-129", "mode-obs1-term0", "chunk-33", "bins-130", "tail-12"])
def test_contract(gpu, name):
    """Runs A / B / C of tests/test_gpu_contract.py: dead cells of log_trans and log_obs dirty (NaN,
    then inf / 1e30 / 88), guards around every tensor, the workspace (8-byte aligned only) zeroed,
    0xFF and stale, the outputs 0xFF, 0x5A and stale."""
    from test_gpu_contract import three_runs
    lib = gpu.load()
    c = _case(name)
    ref = _ref(name)
    B, T, U = c["lt"].shape[:3]
    other = DC.make(B, T, U, c["D"], 4242, obs=c["lo"] is not None)
    ins = {"A": (c["lt"], c["lo"]), "other": (other["lt"], other["lo"]),
           "B": CC.dirty_lattice(c["lt"], c["lo"], c["S"], c["P"], CC.VALUES["nan_ones"], c["terminal"]),
           "C": CC.dirty_lattice(c["lt"], c["lo"], c["S"], c["P"], CC.alternating(B), c["terminal"])}
    inputs = {}
    for run, (lt, lo) in ins.items():
        inputs[run] = {"lt": lt, "sl": c["S"], "pl": c["P"]}
        if lo is not None:
            inputs[run]["lo"] = lo
    wsb = int(lib.ssnt_duration_posterior_workspace_size(B, T, U, c["D"]))
    assert wsb > 0

    def check(got, run):
        _check(gpu, dict(got, status=np.zeros(1, np.int32)), ref, c, f"{name} run {run}", identities=False)

    three_runs(lib, "ssnt_duration_posterior_device", _specs(c, wsb, ws_offset=8), _args(c, wsb), inputs,
               list(DC.OUTPUTS), check)


@pytest.mark.parametrize("name", ["lane-65", "chunk-65", "bins-66", "mode-obs1-term1"])
def test_alone_equals_batch_whatever_the_padding(gpu, name):
    c = _case(name)
    got = _run(gpu, c)
    for b in range(len(c["S"])):
        S, P = int(c["S"][b]), int(c["P"][b])
        for crop in (False, True):
            alone = _run(gpu, _alone(c, b, crop))
            assert CC.same_bits(alone["loss"][0], got["loss"][b]), (name, b, crop)
            n = P if crop else c["lt"].shape[2]
            assert CC.same_bits(alone["dur_post"][0, :n], got["dur_post"][b, :n]), (name, b, crop)


def test_deterministic_and_out_reuse(gpu):
    c = _case("lane-257")
    a, b = _run(gpu, c), _run(gpu, c)
    assert CC.same_bits(a, b)
    B, T, U = c["lt"].shape[:3]
    out = {"dur_post": torch.full((B, U, c["D"]), 7.0, device=DEV), "loss": torch.full((B,), 7.0, device=DEV),
           "status": torch.ones(1, dtype=torch.int32, device=DEV)}
    for _ in range(2):
        assert CC.same_bits(_run(gpu, c, out=out), a)
    assert CC.same_bits(out["dur_post"].cpu().numpy(), a["dur_post"])
    with pytest.raises(ValueError):
        _run(gpu, c, out={"loss": torch.empty(B + 1, device=DEV)})
    with pytest.raises(ValueError):
        _run(gpu, c, D=257)


def test_refused_calls_write_nothing(gpu):
    lib = gpu.load()
    c = _case("mode-obs1-term1")
    B, T, U = c["lt"].shape[:3]
    wsb = int(lib.ssnt_duration_posterior_workspace_size(B, T, U, c["D"]))
    arena, v = G.lay_out(DEV, _specs(c, wsb))
    for k, a in (("lt", c["lt"]), ("sl", c["S"]), ("pl", c["P"]), ("lo", c["lo"])):
        G.put(v[k], a)
    written = list(DC.OUTPUTS) + ["ws", "status"]
    for k in written:
        G.fill_bytes(v[k], 0x5A)
    before = {k: G.get(v[k]) for k in written}
    ok = _args(c, wsb)(v)

    def but(i, x):
        a = list(ok)
        a[i] = x
        return a
    refused = ((but(6, 1025), ERR_UNSUPPORTED), (but(7, 1), ERR_INVALID_ARG), (but(7, 257), ERR_INVALID_ARG),
               (but(8, 2), ERR_INVALID_ARG), (but(8, 3), ERR_INVALID_ARG), (but(9, None), ERR_INVALID_ARG),
               (but(12, wsb - 1), ERR_WORKSPACE), (but(11, None), ERR_WORKSPACE),
               (but(11, v["ws"].data_ptr() + 4), ERR_WORKSPACE))
    for args, code in refused:
        assert G.call(lib, "ssnt_duration_posterior_device", *args) == code, args[4:9]
    torch.cuda.synchronize()
    arena.check()
    for k in written:
        assert CC.same_bits(G.get(v[k]), before[k]), k
    assert lib.ssnt_duration_posterior_workspace_size(B, T, 1025, c["D"]) == 0
    # loss is optional
    v["status"].zero_()
    assert G.call(lib, "ssnt_duration_posterior_device", *but(10, None)) == 0
    torch.cuda.synchronize()
    arena.check()
    assert CC.same_bits(G.get(v["loss"]), before["loss"])
    ref = _ref("mode-obs1-term1")
    assert np.abs(G.get(v["dur_post"]) - ref["dur_post"]).max() <= TOL["dur_post"]
