"""ssnt_viterbi_align_band on the GPU: bit for bit the band-coordinate reference
of tests/band_viterbi_ref.py (which tests/test_band_viterbi_ref.py holds to viterbi_ref.dp on the
embedding), over band widths on either side of every lane count, the band families of the banded
forward-backward, tie-rich inputs, the dense call on the trivial band, the loop band -> best path
-> band, forced paths across several ballots, both storage modes of the decision words, ragged
and infeasible batches, invalid bands, dead cells, workspaces and output modes."""
import functools

import numpy as np
import pytest
import torch

import band_ref as BR
import band_viterbi_ref as BV
import contract_cases as CC
import guarded as G
from gpu_util import DEV, _t, poisoned_runs, switch_point

pytestmark = pytest.mark.gpu

F32 = np.float32
ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE, ERR_BAD_LENGTH, ERR_BAD_BAND = 1, 5, 6, 7, 10
KEYS = ("log_prob", "position", "duration")


def _run(gpu, c, terminal=True, max_pos="P", **kw):
    if max_pos == "P":
        max_pos = int(max(1, np.max(c["P"])))
    r = gpu.ssnt_viterbi_align_band(_t(c["lt"]), _t(c["bs"]), _t(c["S"]), _t(c["P"]), _t(c["lo"]),
                                    terminal_emit=terminal, max_pos=max_pos, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def _ref(c, terminal=True, max_pos=None):
    return BV.dp(c["lt"], c["lo"], c["bs"], c["S"], c["P"], terminal, max_pos)


def _assert_same(r, o, what=""):
    for k in KEYS:
        if k in o and k in r:
            assert CC.same_bits(r[k], o[k]), (what, k, np.argwhere(r[k] != o[k])[:5])


@functools.lru_cache(maxsize=None)
def _case_and_refs(R, obs):
    c = BV.case(R, obs)
    return c, {t: _ref(c, t) for t in (True, False)}


@pytest.mark.parametrize("term", [True, False], ids=["term1", "term0"])
@pytest.mark.parametrize("obs", [False, True], ids=["obs0", "obs1"])
@pytest.mark.parametrize("R", BV.WIDTHS)
def test_bits_of_the_reference(gpu, R, obs, term):
    c, refs = _case_and_refs(R, obs)
    r = _run(gpu, c, term, check=True)
    _assert_same(r, refs[term], (R, obs, term))
    assert set(r) == set(KEYS) | {"status"} and int(r["status"][0]) == 0
    assert np.isfinite(r["log_prob"]).all()


@pytest.mark.parametrize("obs", [False, True], ids=["obs0", "obs1"])
@pytest.mark.parametrize("R", [5, 64, 130])
def test_tie_rich_inputs(gpu, R, obs):
    c = BV.tie_case(R, obs)
    o = _ref(c)
    assert np.isfinite(o["log_prob"]).sum() >= 0.75 * len(c["S"])
    _assert_same(_run(gpu, c, check=True), o, (R, obs))


@pytest.mark.parametrize("U", [1, 7, 64, 80, 200, 256])
def test_the_trivial_band_is_the_dense_call(gpu, U):
    B, T = 3, 40
    lt, lo = BV.synth(B, T, U, True, U)
    S = np.array([40, 33, 21], np.int32)
    P = np.minimum(np.array([min(U, 40), max(1, (2 * U) // 3), 1], np.int32), S)
    c = {"lt": lt, "lo": lo, "bs": np.zeros((B, T), np.int32), "S": S, "P": P}
    for term in (True, False):
        d = gpu.ssnt_viterbi_align(_t(lt), _t(S), _t(P), _t(lo), terminal_emit=term)
        r = _run(gpu, c, term, max_pos=U)
        for k in KEYS:
            assert CC.same_bits(r[k], d[k].cpu().numpy()), (U, term, k)


def _contact(pos, bs, S, P, R):
    out = np.zeros(len(S), np.int32)
    for b in range(len(S)):
        for s in range(int(S[b])):
            p, st = int(pos[b, s]), int(bs[b, s])
            if p >= 0:
                out[b] += (p == st and st > 0) or (p == st + R - 1 and st + R < int(P[b]))
    return out


def test_the_band_around_the_dense_best_path_and_recutting(gpu, oracle):
    B, T, U, R = 4, 40, 30, 8
    lt = oracle.synth_log_trans(B, T, U, seed=21)
    S = np.array([40, 37, 30, 12], np.int32)
    P = np.array([30, 18, 30, 1], np.int32)
    ltd, sl, pl = _t(lt), _t(S), _t(P)
    vit = gpu.ssnt_viterbi_align(ltd, sl, pl)
    bs = gpu.ssnt_band_from_positions(vit["position"], sl, pl, R)
    band = gpu.ssnt_band_gather(ltd, bs, R, float("-inf"))
    r = gpu.ssnt_viterbi_align_band(band, bs, sl, pl, max_pos=U, check=True)
    torch.cuda.synchronize()
    # the band holds the dense best path and drops paths only: the same path, the same bits
    assert torch.equal(r["position"], vit["position"])
    assert torch.equal(r["duration"], vit["duration"])
    assert CC.same_bits(r["log_prob"].cpu().numpy(), vit["log_prob"].cpu().numpy())
    c = {"lt": band.cpu().numpy(), "lo": None, "bs": bs.cpu().numpy(), "S": S, "P": P}
    _assert_same({k: v.cpu().numpy() for k, v in r.items()}, _ref(c, max_pos=U))
    got = gpu.ssnt_band_edge_contact(r["position"], bs, sl, pl, R)
    want = _contact(r["position"].cpu().numpy(), c["bs"], S, P, R)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(gpu.ssnt_band_edge_contact(r["position"].cpu(), bs.cpu(), S, P, R).numpy(), want)
    # re-cut the band from the banded positions: a valid band, and the same path again
    bs2 = gpu.ssnt_band_from_positions(r["position"], sl, pl, R)
    for b in range(B):
        assert BR.is_valid(bs2[b].cpu().numpy(), int(S[b]), int(P[b]), R)
    band2 = gpu.ssnt_band_gather(ltd, bs2, R, float("-inf"))
    r2 = gpu.ssnt_viterbi_align_band(band2, bs2, sl, pl, max_pos=U, check=True)
    assert torch.equal(r2["position"], r["position"]) and torch.equal(r2["duration"], r["duration"])
    assert CC.same_bits(r2["log_prob"].cpu().numpy(), r["log_prob"].cpu().numpy())


def _query(gpu, B, T, R):
    return int(gpu.load().ssnt_viterbi_align_band_workspace_size(B, T, R))


@functools.lru_cache(maxsize=None)
def _switch(gpu):
    return switch_point(lambda T: _query(gpu, 2, T, 8), hi=1 << 14)


def _forced_case(T):
    """S = 200, P = 10, R = 8: all but one path are -inf. Position 4 is held for 140 steps while the
    band moves twice under it (its column goes 4 -> 3 -> 2), so the walk crosses three 64-step
    ballots at a moving column."""
    S, P, R = 200, 10, 8
    enter = {1: 3, 2: 6, 3: 9, 4: 12, 5: 152, 6: 160, 7: 170, 8: 180, 9: 199}  # p -> its first step
    pos = np.zeros(S, np.int64)
    for p, s in enter.items():
        pos[s:] = p
    bs = BR.band_from_moves(T, S, [40, 100])
    assert BR.is_valid(bs, S, P, R) and np.all((bs[:S] <= pos) & (pos < bs[:S] + R))
    lt = np.full((1, T, R, 2), -np.inf, F32)
    rng = np.random.default_rng(T)
    for s in range(S - 1):
        lt[0, s, pos[s] - bs[s], pos[s + 1] - pos[s]] = -rng.random()
    lt[0, S - 1, pos[S - 1] - bs[S - 1], 0] = -0.5
    c = {"lt": lt, "lo": None, "bs": bs[None], "S": np.array([S], np.int32), "P": np.array([P], np.int32)}
    return c, pos


@pytest.mark.parametrize("mode", ["lds", "workspace"])
def test_a_forced_path_across_ballots(gpu, mode):
    n = _switch(gpu)
    T = 256 if mode == "lds" else n + 1
    assert (_query(gpu, 1, T, 8) == 0) == (mode == "lds")
    c, pos = _forced_case(T)
    r = _run(gpu, c, check=True)
    assert np.array_equal(r["position"][0, :200], pos) and np.all(r["position"][0, 200:] == -1)
    assert r["duration"][0].tolist() == np.bincount(pos, minlength=10).tolist()
    assert r["duration"][0, 4] == 140 and np.isfinite(r["log_prob"][0])
    _assert_same(r, _ref(c), mode)


def _long_case(T, seed):
    R, B = 8, 2
    rng = np.random.default_rng(seed)
    S = np.array([T, T - 5], np.int32)
    P = np.array([20, 9], np.int32)
    bs = np.stack([BR.make_band("random", T, int(S[b]), int(P[b]), R, rng) for b in range(B)])
    lt, lo = BV.synth(B, T, R, True, seed)
    return {"lt": lt, "lo": lo, "bs": bs, "S": S, "P": P}


def test_words_in_lds_and_in_the_workspace(gpu):
    n = _switch(gpu)
    # 16 T bytes (band_start, run starts and the words) beside 53 KB of chunk buffers in 160 KiB
    assert 5000 < n < 8000
    for T in (n, n + 1):
        assert (_query(gpu, 2, T, 8) == 0) == (T == n)
        c = _long_case(T, T)
        _assert_same(_run(gpu, c, check=True), _ref(c), T)
    assert _query(gpu, 2, n + 1, 8) == 2 * (n + 1) * 8


def _specs(c, wsb, U):
    B, T, R = c["lt"].shape[:3]
    f, i = torch.float32, torch.int32
    return {"lt": ((B, T, R, 2), f), "lo": ((B, T, R), f), "bs": ((B, T), i), "sl": ((B,), i), "pl": ((B,), i),
            "log_prob": ((B,), f), "position": ((B, T), i), "duration": ((B, U), i),
            "ws": ((max(wsb, 1),), torch.uint8), "status": ((1,), i)}


def _args(c, v, wsb, U, R=None, path=True, flags=1):
    B, T, R0 = c["lt"].shape[:3]
    return [v["lt"], v["lo"], v["bs"], v["sl"], v["pl"], B, T, R0 if R is None else R, U, flags, v["log_prob"],
            v["position"] if path else None, v["duration"] if path else None,
            v["ws"] if wsb and path else None, wsb if path else 0, v["status"], None]


def test_workspace_contents_guards_and_refusals(gpu):
    lib = gpu.load()
    T = _switch(gpu) + 1
    x, other = _long_case(T, 1), _long_case(T, 2)
    wsb, U = _query(gpu, 2, T, 8), 20
    assert wsb > 0
    arena, v = G.lay_out(DEV, _specs(x, wsb, U))

    def put(c):
        for k, a in (("lt", c["lt"]), ("lo", c["lo"]), ("bs", c["bs"]), ("sl", c["S"]), ("pl", c["P"])):
            G.put(v[k], a)
        for k in KEYS:
            G.fill_bytes(v[k], 0xFF)

    name = "ssnt_viterbi_align_band_device"
    runs = poisoned_runs(arena, v, put, lambda: G.call(lib, name, *_args(x, v, wsb, U)), x, other, KEYS)
    ref = _ref(x, max_pos=U)
    for r in runs:
        _assert_same(r, ref)
    # no path: no workspace, the same log_prob bits, nothing else written
    G.fill_bytes(v["log_prob"], 0xFF)
    before = {k: G.get(v[k]) for k in ("position", "duration", "ws")}
    assert G.call(lib, name, *_args(x, v, wsb, U, path=False)) == 0
    torch.cuda.synchronize()
    arena.check()
    assert CC.same_bits(G.get(v["log_prob"]), ref["log_prob"])
    for k in before:
        assert CC.same_bits(G.get(v[k]), before[k]), k
    # refusals write nothing
    written = list(KEYS) + ["ws", "status"]
    for k in written:
        G.fill_bytes(v[k], 0x5A)
    before = {k: G.get(v[k]) for k in written}
    short = _args(x, v, wsb, U)
    short[14] = wsb - 1
    none = _args(x, v, wsb, U)
    none[13] = None
    odd = _args(x, v, wsb, U)
    odd[13] = v["ws"].data_ptr() + 4
    odd[14] = wsb - 4
    no_lp = _args(x, v, wsb, U)
    no_lp[10] = None
    for args, code in ((_args(x, v, wsb, U, R=0), ERR_UNSUPPORTED), (_args(x, v, wsb, U, R=257), ERR_UNSUPPORTED),
                       (_args(x, v, wsb, U, R=-3), ERR_UNSUPPORTED), (short, ERR_WORKSPACE), (none, ERR_WORKSPACE),
                       (odd, ERR_WORKSPACE), (_args(x, v, wsb, U, flags=2), ERR_INVALID_ARG),
                       (_args(x, v, wsb, U, flags=3), ERR_INVALID_ARG), (no_lp, ERR_INVALID_ARG)):
        assert G.call(lib, name, *args) == code
    torch.cuda.synchronize()
    arena.check()
    for k in written:
        assert CC.same_bits(G.get(v[k]), before[k]), k
    assert _query(gpu, 2, T, 0) == 0 and _query(gpu, 2, T, 257) == 0 and _query(gpu, 2, T, -3) == 0


def _alone(gpu, c, b, terminal=True, max_pos="P"):
    one = {k: (None if v is None else v[b:b + 1]) for k, v in c.items()}
    return _run(gpu, one, terminal, max_pos)


def _is_empty(r, b):
    return r["log_prob"][b] == -np.inf and np.all(r["position"][b] == -1) and not r["duration"][b].any()


def test_ragged_batch_with_infeasible_utterances(gpu):
    R, T, U = 8, 30, 17
    rng = np.random.default_rng(11)
    #        ok       S<P     S=0     P=0    -inf      ok        S>T       ok S=P=1  S<0
    SP = [(30, 12), (5, 9), (0, 3), (7, 0), (20, 6), (17, 17), (31, 10), (1, 1), (-2, 3)]
    S = np.array([s for s, _ in SP], np.int32)
    P = np.array([p for _, p in SP], np.int32)
    bs = np.zeros((len(SP), T), np.int32)
    for b in (0, 4):
        bs[b] = BR.make_band("random", T, int(S[b]), int(P[b]), R, rng)
    bs[5] = BR.make_band("diag", T, 17, 17, R)
    lt, lo = BV.synth(len(SP), T, R, True, 5)
    lt[4, 9] = -np.inf  # no path crosses row 9
    c = {"lt": lt, "lo": lo, "bs": bs, "S": S, "P": P}
    for term in (True, False):
        r = _run(gpu, c, term, max_pos=U)
        assert gpu.load().ssnt_status_from_bits(int(r["status"][0])) == ERR_BAD_LENGTH
        _assert_same(r, _ref(c, term, max_pos=U), term)
        for b in range(len(SP)):
            a = _alone(gpu, c, b, term, max_pos=U)
            for k in KEYS:
                assert CC.same_bits(r[k][b:b + 1], a[k]), (b, k)
            assert _is_empty(r, b) == (b in (1, 2, 3, 4, 6, 8)), b
    keep = [b for b in range(len(SP)) if b not in (6, 8)]
    sub = {k: v[keep] for k, v in c.items()}
    r = _run(gpu, sub, max_pos=U)
    assert int(r["status"][0]) == 0
    _assert_same(r, _ref(sub, max_pos=U))


@pytest.mark.parametrize("R", [8, 130])
def test_invalid_bands(gpu, R):
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
    names = list(bad)
    B = len(names) + 2
    bs = np.stack([good] + [bad[n] for n in names] + [good])
    Sv = np.full(B, S, np.int32)
    Pv = np.full(B, P, np.int32)
    Pv[1 + names.index("misses")] = R + 1 if R == 8 else 140  # all-stay misses P - 1 only when P > R
    for n in names:
        b = 1 + names.index(n)
        assert not BR.is_valid(bs[b], int(Sv[b]), int(Pv[b]), R), n
    lt, lo = BV.synth(B, T, R, True, 9)
    c = {"lt": lt, "lo": lo, "bs": bs, "S": Sv, "P": Pv}
    for term in (True, False):
        r = _run(gpu, c, term)
        assert gpu.load().ssnt_status_from_bits(int(r["status"][0])) == ERR_BAD_BAND
        for b in range(1, B - 1):
            assert _is_empty(r, b), names[b - 1]
        for b in (0, B - 1):
            a = _alone(gpu, c, b, term, max_pos=int(Pv.max()))
            assert int(a["status"][0]) == 0
            for k in KEYS:
                assert CC.same_bits(r[k][b:b + 1], a[k]), (b, k)
            assert np.isfinite(r["log_prob"][b])
        _assert_same(r, _ref(c, term), term)
    with pytest.raises(gpu.SsntError) as e:
        gpu.ssnt_viterbi_align_band(_t(lt), _t(bs), _t(Sv), _t(Pv), _t(lo), check=True)
    assert e.value.code == ERR_BAD_BAND and "band" in str(e.value)


@pytest.mark.parametrize("R", [5, 64, 130])
@pytest.mark.parametrize("term", [True, False], ids=["term1", "term0"])
def test_dead_cells_are_never_read(gpu, R, term):
    c = BV.case(R, True, seed=3)
    clean = _run(gpu, c, term)
    _assert_same(clean, _ref(c, term))
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
        r = _run(gpu, d, term)
        assert int(r["status"][0]) == 0
        for k in KEYS:
            assert CC.same_bits(r[k], clean[k]), (name, k)


def test_output_modes(gpu):
    c, refs = _case_and_refs(65, True)
    ref = refs[True]
    B, T = c["bs"].shape
    U = int(c["P"].max())
    out = {"log_prob": torch.full((B,), 7.0, device=DEV),
           "position": torch.full((B, T), 7, dtype=torch.int32, device=DEV),
           "duration": torch.full((B, U), 7, dtype=torch.int32, device=DEV),
           "status": torch.full((1,), 5, dtype=torch.int32, device=DEV)}
    for _ in range(2):
        r = gpu.ssnt_viterbi_align_band(_t(c["lt"]), _t(c["bs"]), _t(c["S"]), _t(c["P"]), _t(c["lo"]),
                                        max_pos=U, out=out)
        assert all(r[k] is out[k] for k in out)
        torch.cuda.synchronize()
        _assert_same({k: v.cpu().numpy() for k, v in r.items()}, ref)
        assert int(out["status"].item()) == 0
    # log_prob alone: the same bits
    r = _run(gpu, c, need_path=False)
    assert set(r) == {"log_prob", "status"} and CC.same_bits(r["log_prob"], ref["log_prob"])
    # position without duration
    r = _run(gpu, c, max_pos=None)
    assert set(r) == {"log_prob", "position", "status"}
    _assert_same(r, ref)
    # a duration too short for some utterances: a bad length for those alone
    small = int(np.sort(np.unique(c["P"]))[-2])
    r = _run(gpu, c, max_pos=small)
    assert gpu.load().ssnt_status_from_bits(int(r["status"][0])) == ERR_BAD_LENGTH
    o = _ref(c, max_pos=small)
    _assert_same(r, o)
    long = c["P"] > small
    assert long.any() and not long.all()
    assert all(_is_empty(r, b) == bool(long[b]) for b in range(B))
    for R_bad in (0, 257):
        with pytest.raises(gpu.SsntError) as e:
            gpu.ssnt_viterbi_align_band(torch.zeros((2, 8, R_bad, 2), device=DEV),
                                        torch.zeros((2, 8), dtype=torch.int32, device=DEV),
                                        torch.ones(2, device=DEV), torch.ones(2, device=DEV))
        assert e.value.code == ERR_UNSUPPORTED
