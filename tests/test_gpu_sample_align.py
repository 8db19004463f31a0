"""GPU posterior sampling on the emit/shift lattice (sample_align.hip) against
the float64 reference of tests/sample_ref.py. Every case checks: each returned path is a valid
monotone path with matching durations; log_prob is bit-equal to the sequential f32 sum of the
returned path; every *clear* sample (reference margin > 1e-4) has exactly the reference's path; the
share of unclear samples stays within the cap that tests/test_sample_ref.py asserts on the CPU."""
import numpy as np
import pytest
import torch

import sample_cases as SC
import sample_ref as SR
import value_cases as VC
from gpu_util import DEV, _t, vp

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED, WORKSPACE, BAD_LENGTH = 1, 5, 6, 7


def _args(c):
    return (_t(c["lt"]), _t(c["S"], torch.int32), _t(c["P"], torch.int32), c["K"],
            None if c["lo"] is None else _t(c["lo"]))


def _run(gpu, c, **kw):
    kw.setdefault("uniform", _t(c["u"]))
    r = gpu.ssnt_sample_align(*_args(c), terminal_emit=c["terminal"], **kw)
    return {k: v.cpu().numpy() for k, v in r.items()}


def _check(c, g, cap=True, where=""):
    lt, lo, S, P, K, ref = c["lt"], c["lo"], c["S"], c["P"], c["K"], c["ref"]
    B, T, U, _ = lt.shape
    assert g["log_prob"].shape == (B, K) and g["log_prob"].dtype == np.float32
    assert g["position"].shape == (B, K, T) and g["position"].dtype == np.int32
    assert g["duration"].shape == (B, K, U) and g["duration"].dtype == np.int32
    for b in range(B):
        s, p = int(S[b]), int(P[b])
        if not ref["feasible"][b]:  # the infeasible rule, every sample
            assert np.all(np.isneginf(g["log_prob"][b])), (where, b)
            assert np.all(g["position"][b] == -1) and np.all(g["duration"][b] == 0), (where, b)
            continue
        pos, dur = g["position"][b], g["duration"][b]
        assert np.all(pos[:, 0] == 0) and np.all(pos[:, s - 1] == p - 1), (where, b)
        assert np.all(np.isin(np.diff(pos[:, :s], axis=1), (0, 1))), (where, b)
        assert np.all(pos[:, s:] == -1) and np.all(dur[:, p:] == 0), (where, b)
        assert np.all(dur.sum(axis=1) == s), (where, b)
        lob = None if lo is None else lo[b]
        for k in range(K):
            assert np.array_equal(np.bincount(pos[k, :s], minlength=U), dur[k]), (where, b, k)
            want = SR.path_log_prob_f32(lt[b], lob, pos[k], c["terminal"])
            assert g["log_prob"][b, k].tobytes() == want.tobytes(), (where, b, k, g["log_prob"][b, k], want)
    clear = ref["clear"]
    wrong = clear & np.any(g["position"] != ref["position"], axis=2)
    assert not wrong.any(), (where, "clear samples off the reference path:", np.argwhere(wrong)[:8].tolist())
    assert np.array_equal(g["duration"][clear], ref["duration"][clear]), where
    unclear, total = SC.unclear_share(c)
    agree = int(np.all(g["position"] == ref["position"], axis=2)[ref["feasible"]].sum())
    print(f"{where}: {unclear} of {total} unclear, {agree} of {total} equal to the reference")
    if cap:
        assert unclear <= SC.CAP_CASE * total, where


@pytest.mark.parametrize("obs,terminal", SC.TINY)
def test_tiny_exhaustive(gpu, obs, terminal):
    c = SC.tiny(obs, terminal)
    _check(c, _run(gpu, c), where=f"tiny {obs} {terminal}")


@pytest.mark.parametrize("U", SC.LANE_WIDTHS)
def test_lane_boundaries(gpu, U):
    c = SC.lane(U)
    _check(c, _run(gpu, c), where=f"lane {U}")


@pytest.mark.parametrize("T", SC.CHUNK_STEPS)
def test_chunk_boundaries(gpu, T):
    c = SC.chunk(T)
    _check(c, _run(gpu, c), where=f"chunk {T}")


@pytest.mark.parametrize("K", SC.K_EDGES)
def test_sample_count_edges(gpu, K):
    c = SC.k_edge(K)
    _check(c, _run(gpu, c), where=f"K {K}")


def test_single_sample_on_a_long_row(gpu):
    # K = 1 at U > 256: the one shape class whose decisions the chain wave takes itself
    c = SC.single_long_row()
    _check(c, _run(gpu, c), where="single long row")


def test_lds_to_workspace_switch(gpu):
    lib = gpu.load()
    Tl = SC.switch_T(lib)
    assert lib.ssnt_sample_align_workspace_size(2, Tl, SC.SWITCH_U, SC.SWITCH_K) == 0
    assert lib.ssnt_sample_align_workspace_size(2, Tl + 1, SC.SWITCH_U, SC.SWITCH_K) > 0
    for T in (Tl, Tl + 1):
        c = SC.switch(T)
        _check(c, _run(gpu, c), where=f"switch {T}")


def test_exponent_range(gpu):
    # T = 2000: alpha falls far below the f32 range; the split exponent must carry it (validity,
    # log_prob bits and clear-sample equality; no cap on the unclear share over 2000 decisions)
    c = SC.exponent_range()
    g = _run(gpu, c)
    # (ln 2^-149 = -103.3: a plain f32 probability of such a path, and alpha along it, would be 0)
    assert np.all(np.isfinite(g["log_prob"])) and np.all(g["log_prob"] < -104)
    _check(c, g, cap=False, where="exponent range")
    assert c["ref"]["clear"].any()


@pytest.mark.parametrize("name", VC.TOLERANCE_CLASSES)
def test_value_classes(gpu, name):
    # saturated, positive, exponent-heavy and alternating inputs (tests/value_cases.py): the same
    # checks as every other case, the cap included
    c = SC.value(name)
    _check(c, _run(gpu, c), where=f"value {name}")


def test_zero_probability_transitions(gpu):
    c = SC.zero_probability()
    ref = c["ref"]
    assert not ref["feasible"][0] and 8 <= int(ref["feasible"].sum()) < len(ref["feasible"])
    g = _run(gpu, c)
    _check(c, g, where="zero probability")
    # no drawn path crosses a -inf entry: log_prob is finite unless the terminal emit itself is -inf
    # (alpha[S-1][P-1] > 0 makes the utterance feasible; the terminal emit is common to all paths)
    for b in np.nonzero(ref["feasible"])[0]:
        end = np.isfinite(c["lt"][b, c["S"][b] - 1, c["P"][b] - 1, 0])
        assert np.all(np.isfinite(g["log_prob"][b]) == end), b


def test_frequency_on_the_gpu(gpu):
    c = SC.frequency()
    g = _run(gpu, c)
    _check(c, g, where="frequency")
    post = SR.path_posterior(c["lt"][0], 7, 3, c["lo"][0])
    dev = SR.frequency_deviation(g["position"].reshape(-1, 7), 7, post)
    print("deviation in sigma:", dev)
    assert dev <= 5.0


def test_clamping(gpu):
    B, T, U, K = 3, 12, 5, 4
    lt1, _ = SC.lattice(1, T, U, 9)
    lt = np.repeat(lt1, B, axis=0)
    u = np.empty((B, K, T), np.float32)
    u[0], u[1], u[2] = 1.0, np.nan, -1.0
    uc = np.empty_like(u)
    uc[0], uc[1], uc[2] = SR.U_MAX, 0.0, 0.0
    c = SC._case(lt, None, [T] * B, [U] * B, K, 0, u=uc)  # the reference run with the clamped values
    # u = 1 - 2^-24 moves only where it must: clear by the margin. u = 0 moves wherever the move
    # term is positive, which f32 and float64 agree on while rho is far above 2^-149
    assert c["ref"]["clear"][0].all()
    one = SR.sample(lt[1], T, U, uc[1])
    assert one["rho"][one["rho"] > 0].min() > 1e-30
    g = _run(gpu, c, uniform=_t(u))
    _check(c, g, cap=False, where="clamping")
    assert np.array_equal(g["position"], c["ref"]["position"])
    assert np.array_equal(g["duration"], c["ref"]["duration"])
    assert np.array_equal(g["position"][1], g["position"][2])


def test_errors(gpu):
    lib = gpu.load()
    c = SC.reuse()
    B, T, U, _ = c["lt"].shape
    K = c["K"]
    x, s, p, _, o = _args(c)
    un = _t(c["u"])
    lp = torch.full((B, 64), 7.0, device=DEV)
    pos = torch.full((B, 64, T), 9, dtype=torch.int32, device=DEV)
    dur = torch.full((B, 64, U), 9, dtype=torch.int32, device=DEV)
    st = torch.zeros(1, dtype=torch.int32, device=DEV)

    def call(lt=x, sl=s, pl=p, u=un, b=B, t=T, w=U, k=K, flags=1, out=lp, ws=None, wsb=0):
        return lib.ssnt_sample_align_device(vp(lt), vp(o), vp(sl), vp(pl), vp(u), b, t, w, k, flags,
                                            vp(out), vp(pos), vp(dur), vp(ws), wsb, vp(st), None)

    assert call(k=0) == INVALID and call(k=65) == INVALID and call(k=-1) == INVALID
    assert call(w=1025) == UNSUPPORTED
    assert call(flags=2) == INVALID and call(flags=3) == INVALID
    assert call(lt=None) == INVALID and call(sl=None) == INVALID and call(pl=None) == INVALID
    assert call(u=None) == INVALID and call(out=None) == INVALID
    assert call(b=-1) == INVALID and call(t=-1) == INVALID and call(w=-1) == INVALID
    assert call(b=0) == 0
    # a shape whose bits need the workspace: missing / too small
    Tw = SC.switch_T(lib) + 1
    cw = SC.switch(Tw)
    xw, sw, pw, Kw, ow = _args(cw)
    need = int(lib.ssnt_sample_align_workspace_size(2, Tw, SC.SWITCH_U, Kw))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    uw = _t(cw["u"])
    lpw = torch.empty((2, Kw), device=DEV)

    def callw(ws=None, wsb=0, out=lp):
        return lib.ssnt_sample_align_device(vp(xw), vp(ow), vp(sw), vp(pw), vp(uw), 2, Tw, SC.SWITCH_U,
                                            Kw, 1, vp(out), None, None, vp(ws), wsb, vp(st), None)

    assert callw() == WORKSPACE and callw(ws, need - 1) == WORKSPACE
    torch.cuda.synchronize()
    # none of the refused calls touched an output
    assert bool(torch.all(lp == 7.0)) and bool(torch.all(pos == 9)) and bool(torch.all(dur == 9))
    assert int(st.item()) == 0
    assert callw(ws, need, lpw) == 0
    torch.cuda.synchronize()
    got = lpw.cpu().numpy()
    for b, k in np.argwhere(cw["ref"]["clear"]):  # with the workspace the call runs: log_prob only
        want = SR.path_log_prob_f32(cw["lt"][b], cw["lo"][b], cw["ref"]["position"][b, k], True)
        assert got[b, k].tobytes() == want.tobytes(), (b, k)
    assert bool(torch.all(pos == 9)) and bool(torch.all(dur == 9))


def test_bad_length_status(gpu):
    B, T, U, K = 4, 10, 4, 8
    lt, _ = SC.lattice(B, T, U, 8)
    c = SC._case(lt, None, [10, 11, 8, 10], [4, 4, 5, 2], K, 2)  # [1]: S > T, [2]: P > U
    assert c["ref"]["feasible"].tolist() == [True, False, False, True]
    g = _run(gpu, c, check=False)
    _check(c, g, cap=False, where="bad length")
    assert gpu.load().ssnt_status_from_bits(int(g["status"][0])) == BAD_LENGTH
    with pytest.raises(gpu.SsntError) as e:
        _run(gpu, c)
    assert e.value.code == BAD_LENGTH


def test_need_path_false_and_out_reuse(gpu):
    c = SC.reuse()
    B, T, U, _ = c["lt"].shape
    K = c["K"]
    g = _run(gpu, c)
    _check(c, g, where="reuse")
    assert np.array_equal(g["uniform"], c["u"])
    n = _run(gpu, c, need_path=False)
    assert set(n) == {"log_prob", "uniform", "status"}
    assert n["log_prob"].tobytes() == g["log_prob"].tobytes()
    out = {"log_prob": torch.full((B, K), 7.0, device=DEV),
           "position": torch.full((B, K, T), 9, dtype=torch.int32, device=DEV),
           "duration": torch.full((B, K, U), 9, dtype=torch.int32, device=DEV),
           "status": torch.ones(1, dtype=torch.int32, device=DEV)}
    r = gpu.ssnt_sample_align(*_args(c), uniform=_t(c["u"]), out=out)
    for k in out:
        assert r[k].data_ptr() == out[k].data_ptr()
        assert np.array_equal(r[k].cpu().numpy(), g[k]), k
    with pytest.raises(ValueError):
        gpu.ssnt_sample_align(*_args(c), out={"position": torch.empty((B, K, T), dtype=torch.int64, device=DEV)})
    with pytest.raises(ValueError):
        gpu.ssnt_sample_align(*_args(c), uniform=torch.zeros((B, K + 1, T), device=DEV))
    # without `uniform` the numbers come from the generator and are returned; the same numbers
    # give the same paths
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    a = gpu.ssnt_sample_align(*_args(c), generator=gen)
    assert a["uniform"].shape == (B, K, T) and a["uniform"].dtype == torch.float32
    assert float(a["uniform"].min()) >= 0 and float(a["uniform"].max()) < 1
    b = gpu.ssnt_sample_align(*_args(c), uniform=a["uniform"])
    assert torch.equal(a["position"], b["position"]) and torch.equal(a["log_prob"], b["log_prob"])
    gen.manual_seed(5)
    a2 = gpu.ssnt_sample_align(*_args(c), generator=gen)
    assert torch.equal(a["uniform"], a2["uniform"]) and torch.equal(a["position"], a2["position"])


def test_two_streams(gpu):
    # one LDS shape and one workspace shape, concurrently on two streams = the serial results
    ca, cb = SC.reuse(), SC.switch(SC.switch_T(gpu.load()) + 1)
    ga, gb = _run(gpu, ca), _run(gpu, cb)
    aa, ab, ua, ub = _args(ca), _args(cb), _t(ca["u"]), _t(cb["u"])
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(2):
        with torch.cuda.stream(s1):
            ra = gpu.ssnt_sample_align(*aa, uniform=ua, check=False)
        with torch.cuda.stream(s2):
            rb = gpu.ssnt_sample_align(*ab, uniform=ub, check=False)
    torch.cuda.synchronize()
    for r, g in ((ra, ga), (rb, gb)):
        for k in ("log_prob", "position", "duration"):
            assert np.array_equal(r[k].cpu().numpy(), g[k]), k
        assert int(r["status"].item()) == 0
