"""ssnt_fwd_bwd_band on the GPU: bit for bit the oracle on the embedding of the
band into a dense lattice (tests/band_ref.py), over band widths on either side of every lane
count, band families that move everywhere around the cut, input value classes, ragged and
infeasible batches, invalid bands, dead cells, workspaces and output modes."""
import functools

import numpy as np
import pytest
import torch

import band_ref as BR
import contract_cases as CC
import guarded as G
import value_cases as VC
from gpu_util import DEV, _t, poisoned_runs, switch_point

pytestmark = pytest.mark.gpu

F32 = np.float32
ERR_UNSUPPORTED, ERR_BAD_LENGTH, ERR_BAD_BAND = 5, 7, 10
WIDTHS = (1, 2, 3, 5, 63, 64, 65, 128, 130, 256)
FLAGS = {"term": 1, "none": 0, "term-zinf": 3}
T0 = 48


def log_tol(x):
    return 1e-5 + 2.0 ** -23 * abs(float(x))


def _synth(oracle, B, T, R, obs, seed):
    lt = oracle.synth_log_trans(B, T, R, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    lo = (rng.standard_normal((B, T, R)) * 15 - 40).astype(F32) if obs else None
    return lt, lo


def _utterances(R):
    """(S, P, kind, at) of the batch every width runs; families a shape has no band for drop out."""
    M = 20  # of S = 41
    P1 = min(R + 1, 30)
    return [(48, min(R, 40), "stay", None), (48, 48, "diag", None), (45, 45, "diag", None),
            (33, 33, "diag", None), (25, 25, "diag", None), (47, 30, "alt", None),
            (45, 20, "random", None), (38, 37, "random", None), (41, P1, "at", M - 1),
            (41, P1, "at", M), (41, P1, "at", M + 1), (1, 1, "stay", None),
            (30, max(1, min(R // 2, 30)), "stay", None), (48, min(R + 7, 48), "random", None)]


@functools.lru_cache(maxsize=None)
def _bands(R):
    rng = np.random.default_rng(R)
    rows = []
    for S, P, kind, at in _utterances(R):
        bs = BR.make_band(kind, T0, S, P, R, rng, at)
        if bs is not None:
            assert BR.is_valid(bs, S, P, R)
            rows.append((S, P, bs))
    S = np.array([r[0] for r in rows], np.int32)
    P = np.array([r[1] for r in rows], np.int32)
    return S, P, np.stack([r[2] for r in rows])


def _case(oracle, R, obs, seed=0):
    S, P, bs = _bands(R)
    lt, lo = _synth(oracle, len(S), T0, R, obs, seed + R)
    return {"lt": lt, "lo": lo, "bs": bs, "S": S, "P": P}


def _run(gpu, c, flags=1, **kw):
    r = gpu.ssnt_fwd_bwd_band(_t(c["lt"]), _t(c["bs"]), _t(c["S"]), _t(c["P"]), _t(c["lo"]),
                              terminal_emit=bool(flags & 1), zero_infinity=bool(flags & 2), **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def _ref(oracle, c, flags=1):
    o = BR.oracle_band(oracle, c["lt"], c["lo"], c["bs"], c["S"], c["P"], flags=flags)
    return {k: o[k] for k in ("loss", "grad", "grad_obs") if k in o}


def _assert_same(r, o, what=""):
    for k in o:
        assert CC.same_bits(r[k], o[k]), (what, k, np.argwhere(r[k].view(np.uint32) != o[k].view(np.uint32))[:5])


def test_the_cut_meets_every_block_alignment():
    # band_start[M] % R' zero and non-zero, base / R' odd and even, a band across two blocks at M
    seen = set()
    for R in WIDTHS:
        Rp = 1 << (R - 1).bit_length()
        S, P, bs = _bands(R)
        for b in range(len(S)):
            st = int(bs[b, (S[b] - 1) >> 1])
            seen.add((st % Rp == 0, (st // Rp) % 2, st % Rp + min(R, P[b] - st) > Rp))
    assert {(z, o) for z, o, _ in seen} == {(True, 0), (True, 1), (False, 0), (False, 1)}
    assert any(x for _, _, x in seen)


@pytest.mark.parametrize("flags", list(FLAGS), ids=list(FLAGS))
@pytest.mark.parametrize("obs", [False, True], ids=["obs0", "obs1"])
@pytest.mark.parametrize("R", WIDTHS)
def test_bits_of_the_oracle_on_the_embedding(gpu, oracle, R, obs, flags):
    c = _case(oracle, R, obs)
    r = _run(gpu, c, FLAGS[flags], check=True)
    _assert_same(r, _ref(oracle, c, FLAGS[flags]), (R, obs, flags))
    assert int(r["status"][0]) == 0


def test_width_one_is_the_single_path(gpu, oracle):
    T, S = 20, 17
    rng = np.random.default_rng(3)
    for P in (1, 9, 17):
        bs = BR.make_band("random", T, S, P, 1, rng)[None]
        lt, lo = _synth(oracle, 1, T, 1, True, P)
        c = {"lt": lt, "lo": lo, "bs": bs, "S": np.array([S], np.int32), "P": np.array([P], np.int32)}
        r = _run(gpu, c)
        _assert_same(r, _ref(oracle, c), P)
        mv = np.diff(bs[0, :S])
        total = float(np.sum(lo[0, :S, 0], dtype=np.float64) + lt[0, S - 1, 0, 0]
                      + np.sum(np.where(mv == 1, lt[0, :S - 1, 0, 1], lt[0, :S - 1, 0, 0]), dtype=np.float64))
        assert abs(float(r["loss"][0]) + total) <= log_tol(total) * S
        want = np.zeros((T, 1, 2))
        want[np.arange(S - 1), 0, mv] = -1.0
        want[S - 1, 0, 0] = -1.0
        assert np.abs(r["grad"][0] - want).max() <= 1e-5
        assert np.abs(r["grad_obs"][0, :S, 0] + 1.0).max() <= 1e-5 and not r["grad_obs"][0, S:].any()


def _value_case(oracle, R, name, kind, obs_name=None):
    B, T = 4, 40
    U = 20 if R == 8 else 150
    S, P = VC.lengths(B, T, min(U, R + 12), kind)
    rng = np.random.default_rng(R)
    bs = np.stack([BR.make_band("diag" if S[b] == P[b] else "random", T, int(S[b]), int(P[b]), R, rng)
                   for b in range(B)])
    base = oracle.synth_log_trans(B, T, R, seed=7)
    lt = VC.lattice(name, base, seed=R)
    lo = None if obs_name is None else VC.obs(obs_name, (B, T, R), seed=R)
    return {"lt": lt, "lo": lo, "bs": bs, "S": S, "P": P}


@pytest.mark.parametrize("R", [8, 130])
@pytest.mark.parametrize("name", VC.LATTICE_CLASSES)
def test_value_classes(gpu, oracle, name, R):
    for kind in VC.length_kinds(name):
        c = _value_case(oracle, R, name, kind)
        _assert_same(_run(gpu, c), _ref(oracle, c), (name, kind))


@pytest.mark.parametrize("trans", ["peaked10", "peaked30"])
@pytest.mark.parametrize("name", list(VC.OBS))
def test_obs_value_classes(gpu, oracle, name, trans):
    c = _value_case(oracle, 8, trans, "ragged", obs_name=name)
    _assert_same(_run(gpu, c), _ref(oracle, c), (name, trans))


def test_near_the_exponent_envelope(gpu, oracle):
    B, T, R = VC.NEAR_ENVELOPE["shape"]
    S, P = np.array(VC.NEAR_ENVELOPE["S"], np.int32), np.array(VC.NEAR_ENVELOPE["P"], np.int32)
    c = {"lt": VC.lattice("near_envelope", oracle.synth_log_trans(B, T, R, seed=1)), "lo": None,
         "bs": np.zeros((B, T), np.int32), "S": S, "P": P}
    _assert_same(_run(gpu, c), _ref(oracle, c))


@pytest.mark.parametrize("U", [1, 7, 64, 80, 200, 256])
def test_the_trivial_band_is_the_dense_call(gpu, oracle, U):
    B, T = 3, 40
    lt, lo = _synth(oracle, B, T, U, True, U)
    S = np.array([40, 33, 21], np.int32)
    P = np.minimum(np.array([min(U, 40), max(1, (2 * U) // 3), 1], np.int32), S)
    c = {"lt": lt, "lo": lo, "bs": np.zeros((B, T), np.int32), "S": S, "P": P}
    for flags in (1, 0):
        d = gpu.ssnt_fwd_bwd(_t(lt), _t(S), _t(P), _t(lo), terminal_emit=bool(flags))
        r = _run(gpu, c, flags)
        for k in ("loss", "grad", "grad_obs"):
            assert CC.same_bits(r[k], d[k].cpu().numpy()), (U, flags, k)


def _alone(gpu, c, b, flags=1):
    one = {k: (None if v is None else v[b:b + 1]) for k, v in c.items()}
    return _run(gpu, one, flags)


def test_ragged_batch_with_infeasible_utterances(gpu, oracle):
    R, T = 8, 30
    rng = np.random.default_rng(11)
    #        ok       S<P     S=0     P=0     Z=0      ok        S>T       ok S=P=1
    SP = [(30, 12), (5, 9), (0, 3), (7, 0), (20, 6), (17, 17), (31, 10), (1, 1)]
    S = np.array([s for s, _ in SP], np.int32)
    P = np.array([p for _, p in SP], np.int32)
    bs = np.zeros((len(SP), T), np.int32)
    for b in (0, 4):
        bs[b] = BR.make_band("random", T, int(S[b]), int(P[b]), R, rng)
    bs[5] = BR.make_band("diag", T, 17, 17, R)
    lt, lo = _synth(oracle, len(SP), T, R, True, 5)
    lt[4, 9] = -np.inf  # no path crosses row 9
    c = {"lt": lt, "lo": lo, "bs": bs, "S": S, "P": P}
    for flags in (1, 3):
        r = _run(gpu, c, flags)
        assert gpu.load().ssnt_status_from_bits(int(r["status"][0])) == ERR_BAD_LENGTH
        inf = 0.0 if flags & 2 else np.inf
        for b in range(len(SP)):
            a = _alone(gpu, c, b, flags)
            for k in ("loss", "grad", "grad_obs"):
                assert CC.same_bits(r[k][b:b + 1], a[k]), (b, k)
            if b in (1, 2, 3, 4, 6):
                assert r["loss"][b] == inf and not r["grad"][b].any() and not r["grad_obs"][b].any()
            else:
                assert np.isfinite(r["loss"][b]) and r["loss"][b] != 0
    keep = [b for b in range(len(SP)) if b != 6]
    sub = {k: v[keep] for k, v in c.items()}
    r = _run(gpu, sub)
    assert int(r["status"][0]) == 0
    good = [0, 4, 5]  # (the oracle takes the feasible ones; Z = 0 is among them)
    ok = {k: v[good] for k, v in c.items()}
    _assert_same({k: v[[0, 4, 5]] for k, v in r.items() if k != "status"}, _ref(oracle, ok))


@pytest.mark.parametrize("R", [8, 130])
def test_invalid_bands(gpu, oracle, R):
    T, S, P = 24, 22, 12 if R == 8 else 20
    rng = np.random.default_rng(R)
    good = BR.make_band("random", T, S, P, R, rng)
    if R == 130:
        good = BR.make_band("at", T, S, P, R, rng, at=10)
    bad = {}
    bad["start"] = good + 1
    bad["step2"] = good.copy()
    bad["step2"][7:] += 2
    bad["back"] = good.copy()
    bad["back"][9:] += 1
    bad["back"][12:] -= 2
    bad["misses"] = np.zeros(T, np.int32)  # the last window ends before P - 1 ...
    bad["beyond"] = BR.band_from_moves(T, S, range(S - 1))  # ... or starts after it
    bad["negative"] = good.copy()
    bad["negative"][0] = -1
    bad["huge"] = good.copy()
    bad["huge"][S - 1] = BR.INT_MAX
    bad["lowest"] = good.copy()
    bad["lowest"][3] = BR.INT_MIN
    Pm = P if R == 8 else 140  # all-stay misses P - 1 only when P > R
    names = list(bad)
    B = len(names) + 2
    bs = np.stack([good] + [bad[n] for n in names] + [good])
    Sv = np.full(B, S, np.int32)
    Pv = np.full(B, P, np.int32)
    Pv[1 + names.index("misses")] = Pm if Pm > R else R + 1
    Sv[1 + names.index("misses")] = S
    for n in names:
        b = 1 + names.index(n)
        assert not BR.is_valid(bs[b], int(Sv[b]), int(Pv[b]), R), n
    lt, lo = _synth(oracle, B, T, R, True, 9)
    c = {"lt": lt, "lo": lo, "bs": bs, "S": Sv, "P": Pv}
    for flags in (1, 3):
        r = _run(gpu, c, flags)
        assert gpu.load().ssnt_status_from_bits(int(r["status"][0])) == ERR_BAD_BAND
        for b in range(1, B - 1):
            assert r["loss"][b] == (0.0 if flags & 2 else np.inf), names[b - 1]
            assert not r["grad"][b].view(np.uint32).any() and not r["grad_obs"][b].view(np.uint32).any()
        for b in (0, B - 1):
            a = _alone(gpu, c, b, flags)
            assert int(a["status"][0]) == 0
            for k in ("loss", "grad", "grad_obs"):
                assert CC.same_bits(r[k][b:b + 1], a[k]), (b, k)
    ends = {k: v[[0, B - 1]] for k, v in c.items()}
    _assert_same({k: v[[0, B - 1]] for k, v in r.items() if k != "status"}, _ref(oracle, ends, 3))
    with pytest.raises(gpu.SsntError) as e:
        gpu.ssnt_fwd_bwd_band(_t(lt), _t(bs), _t(Sv), _t(Pv), _t(lo), check=True)
    assert e.value.code == ERR_BAD_BAND and "band" in str(e.value)


@pytest.mark.parametrize("R", [5, 64, 130])
@pytest.mark.parametrize("term", [True, False], ids=["term1", "term0"])
def test_dead_cells_are_never_read(gpu, oracle, R, term):
    c = _case(oracle, R, True, seed=3)
    flags = 1 if term else 0
    clean = _run(gpu, c, flags)
    _assert_same(clean, _ref(oracle, c, flags))
    mt, mo = BR.dead_mask(c["bs"], c["S"], c["P"], R, term)
    assert mt.any() and mo.any() and not mt.all()
    B, T = c["bs"].shape
    beyond = np.arange(T)[None, :] >= c["S"][:, None]
    for i, (name, v) in enumerate(CC.VALUES.items()):
        d = dict(c)
        d["lt"], d["lo"] = c["lt"].copy(), c["lo"].copy()
        d["lt"][mt] = v
        d["lo"][mo] = v
        d["bs"] = np.where(beyond, BR.INT_MIN if i % 2 else BR.INT_MAX, c["bs"]).astype(np.int32)
        r = _run(gpu, d, flags)
        assert int(r["status"][0]) == 0
        for k in ("loss", "grad", "grad_obs"):
            assert CC.same_bits(r[k], clean[k]), (name, k)


def _query(gpu, B, T, R):
    return int(gpu.load().ssnt_fwd_bwd_band_workspace_size(B, T, R))


def _long_case(oracle, T, seed):
    R, B = 8, 2
    rng = np.random.default_rng(seed)
    S = np.array([T, T - 5], np.int32)
    P = np.array([20, 9], np.int32)
    bs = np.stack([BR.make_band("random", T, int(S[b]), int(P[b]), R, rng) for b in range(B)])
    lt, lo = _synth(oracle, B, T, R, True, seed)
    return {"lt": lt, "lo": lo, "bs": bs, "S": S, "P": P}


def test_rows_in_lds_and_in_the_workspace(gpu, oracle):
    n = switch_point(lambda T: _query(gpu, 1, T, 8), hi=8192)
    assert 1000 < n < 2600  # 64 T bytes of rows and 4 T of band_start beside the head in 160 KiB
    for T in (n, n + 1):
        assert (_query(gpu, 2, T, 8) == 0) == (T == n)
        assert _query(gpu, 2, n + 1, 8) == 2 * (n + 1) * 8 * 8
        c = _long_case(oracle, T, T)
        _assert_same(_run(gpu, c), _ref(oracle, c), T)


def _specs(c, wsb):
    B, T, R = c["lt"].shape[:3]
    f, i = torch.float32, torch.int32
    return {"lt": ((B, T, R, 2), f), "lo": ((B, T, R), f), "bs": ((B, T), i), "sl": ((B,), i), "pl": ((B,), i),
            "loss": ((B,), f), "grad": ((B, T, R, 2), f), "grad_obs": ((B, T, R), f),
            "ws": ((max(wsb, 1),), torch.uint8), "status": ((1,), i)}


def _args(c, v, wsb, R=None, grads=True):
    B, T, R0 = c["lt"].shape[:3]
    return [v["lt"], v["lo"], v["bs"], v["sl"], v["pl"], B, T, R0 if R is None else R, 1, v["loss"],
            v["grad"] if grads else None, v["grad_obs"] if grads else None,
            v["ws"] if wsb and grads else None, wsb if grads else 0, v["status"], None]


def test_workspace_contents_and_guards(gpu, oracle):
    lib = gpu.load()
    n = switch_point(lambda T: _query(gpu, 1, T, 8), hi=8192)
    T = n + 1
    x, other = _long_case(oracle, T, 1), _long_case(oracle, T, 2)
    wsb = _query(gpu, 2, T, 8)
    assert wsb > 0
    arena, v = G.lay_out(DEV, _specs(x, wsb))

    def put(c):
        for k, a in (("lt", c["lt"]), ("lo", c["lo"]), ("bs", c["bs"]), ("sl", c["S"]), ("pl", c["P"])):
            G.put(v[k], a)
        for k in ("loss", "grad", "grad_obs"):
            G.fill_bytes(v[k], 0xFF)

    keys = ("loss", "grad", "grad_obs")
    runs = poisoned_runs(arena, v, put, lambda: G.call(lib, "ssnt_fwd_bwd_band_device", *_args(x, v, wsb)),
                         x, other, keys)
    ref = _ref(oracle, x)
    for r in runs:
        _assert_same(r, ref)
    # no gradient: no workspace, the same loss bits
    G.fill_bytes(v["loss"], 0xFF)
    before = {k: G.get(v[k]) for k in ("grad", "grad_obs", "ws")}
    assert G.call(lib, "ssnt_fwd_bwd_band_device", *_args(x, v, wsb, grads=False)) == 0
    torch.cuda.synchronize()
    arena.check()
    assert CC.same_bits(G.get(v["loss"]), ref["loss"])
    for k in before:
        assert CC.same_bits(G.get(v[k]), before[k]), k
    # refusals write nothing: widths outside [1, 256], a short or missing workspace
    written = list(keys) + ["ws", "status"]
    for k in written:
        G.fill_bytes(v[k], 0x5A)
    before = {k: G.get(v[k]) for k in written}
    short = _args(x, v, wsb)
    short[13] = wsb - 1
    none = _args(x, v, wsb)
    none[12] = None
    for args, code in ((_args(x, v, wsb, R=0), ERR_UNSUPPORTED), (_args(x, v, wsb, R=257), ERR_UNSUPPORTED),
                       (_args(x, v, wsb, R=-3), ERR_UNSUPPORTED), (short, 6), (none, 6)):
        assert G.call(lib, "ssnt_fwd_bwd_band_device", *args) == code
    torch.cuda.synchronize()
    arena.check()
    for k in written:
        assert CC.same_bits(G.get(v[k]), before[k]), k
    assert _query(gpu, 2, T, 0) == 0 and _query(gpu, 2, T, 257) == 0


def test_out_reuse_need_grad_and_refused_widths(gpu, oracle):
    c = _case(oracle, 65, True)
    ref = _ref(oracle, c)
    B, T, R = c["lt"].shape[:3]
    out = {"loss": torch.full((B,), 7.0, device=DEV), "grad": torch.full((B, T, R, 2), 7.0, device=DEV),
           "grad_obs": torch.full((B, T, R), 7.0, device=DEV),
           "status": torch.full((1,), 5, dtype=torch.int32, device=DEV)}
    for _ in range(2):
        r = gpu.ssnt_fwd_bwd_band(_t(c["lt"]), _t(c["bs"]), _t(c["S"]), _t(c["P"]), _t(c["lo"]), out=out)
        assert all(r[k] is out[k] for k in out)
        torch.cuda.synchronize()
        _assert_same({k: v.cpu().numpy() for k, v in r.items()}, ref)
        assert int(out["status"].item()) == 0
    r = _run(gpu, c, need_grad=False)
    assert set(r) == {"loss", "status"} and CC.same_bits(r["loss"], ref["loss"])
    for R_bad in (0, 257):
        with pytest.raises(gpu.SsntError) as e:
            gpu.ssnt_fwd_bwd_band(torch.zeros((2, 8, R_bad, 2), device=DEV), torch.zeros((2, 8), dtype=torch.int32, device=DEV),
                                  torch.ones(2, device=DEV), torch.ones(2, device=DEV))
        assert e.value.code == ERR_UNSUPPORTED


def test_autograd_and_the_band_around_the_best_path(gpu, oracle):
    B, T, U, R = 4, 40, 30, 8
    lt = oracle.synth_log_trans(B, T, U, seed=21)
    S = np.array([40, 37, 30, 12], np.int32)
    P = np.array([30, 18, 30, 1], np.int32)
    ltd, sl, pl = _t(lt), _t(S), _t(P)
    vit = gpu.ssnt_viterbi_align(ltd, sl, pl)
    bs = gpu.ssnt_band_from_positions(vit["position"], sl, pl, R)
    for b in range(B):
        assert BR.is_valid(bs[b].cpu().numpy(), int(S[b]), int(P[b]), R)
    band = gpu.ssnt_band_gather(ltd, bs, R, float("-inf")).requires_grad_(True)
    w = torch.tensor([1.0, -2.0, 0.5, 3.0], device=DEV)
    loss = gpu.ssnt_band_lattice_loss(band, bs, sl, pl)
    (loss * w).sum().backward()
    r = gpu.ssnt_fwd_bwd_band(band.detach(), bs, sl, pl)
    torch.cuda.synchronize()
    assert torch.equal(loss.detach(), r["loss"])
    assert torch.equal(band.grad, r["grad"] * w[:, None, None, None])
    dense = gpu.ssnt_fwd_bwd(ltd, sl, pl, need_grad=False)["loss"].cpu().numpy()
    banded, best = r["loss"].cpu().numpy(), -vit["log_prob"].cpu().numpy()
    for b in range(B):
        print(f"utterance {b}: dense {dense[b]:.6f} banded {banded[b]:.6f} best path {best[b]:.6f}")
        assert dense[b] <= banded[b] + log_tol(banded[b]) and banded[b] <= best[b] + log_tol(best[b])
    # the gradient scattered back is the dense layout's, zero outside the band
    back = gpu.ssnt_band_scatter(r["grad"], bs, U)
    assert tuple(back.shape) == (B, T, U, 2)
    # an invalid band is reported in backward
    bad = bs.clone()
    bad[1, 0] = 1
    band2 = band.detach().clone().requires_grad_(True)
    out = gpu.ssnt_band_lattice_loss(band2, bad, sl, pl, None, True, True)
    with pytest.raises(gpu.SsntError):
        out.sum().backward()
