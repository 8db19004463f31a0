"""GPU exact N best duration paths on the v2 lattice (v2_nbest_align.hip)
against the numpy-f32 DP of tests/v2_nbest_ref.py: log_prob bit-identical (tobytes),
duration_class, duration, total and count value-identical (np.array_equal), on both cell forms,
every class padding, the unrolled and the rolled class loop, both backpointer stores and both
entry widths, tie-rich and edge inputs, at the configs[4] row shape, plus N = 1 against
v2_viterbi_align, the independence of a rank from the list width, invariants that do not use the
DP, and the API / error paths."""
import functools

import numpy as np
import pytest
import torch

import f4_cases
import guarded as G
import v2_nbest_ref as NR
import v2_viterbi_ref as VR
from gpu_util import DEV, poisoned_runs, switch_point, _t, vp
from test_gpu_v2_viterbi import F4_TABLES, _edge_inputs, _medium, _softmax_logits

pytestmark = pytest.mark.gpu

KEYS = ("duration_class", "duration", "total")
OUTS = ("log_prob",) + KEYS


def _run(gpu, logits, table, I, O, max_total, N, zid=0, allow_skip=True, test_mode=False, **kw):
    r = gpu.v2_nbest_align(_t(np.asarray(logits, np.float32)), _t(np.asarray(table), torch.int32),
                           _t(np.asarray(I), torch.int32), _t(np.asarray(O), torch.int32), zid, N,
                           allow_skip=allow_skip, test_mode=test_mode, max_total=max_total, **kw)
    return {k: v.cpu().numpy() for k, v in r.items()}


def _same(g, ref, where=""):
    assert g["log_prob"].dtype == np.float32 and g["log_prob"].shape == ref["log_prob"].shape
    assert g["log_prob"].tobytes() == ref["log_prob"].tobytes(), (where, g["log_prob"], ref["log_prob"])
    for k in KEYS:
        assert g[k].dtype == np.int32 and np.array_equal(g[k], ref[k]), (where, k)
    if "count" in g:
        assert g["count"].dtype == np.int32 and np.array_equal(g["count"], ref["count"]), where


def _first(r, n):
    """The first n ranks of a result."""
    out = {k: np.ascontiguousarray(r[k][:, :n]) for k in OUTS}
    out["count"] = np.minimum(r["count"], n).astype(np.int32)
    return out


def _check_absent(g, b, n0=0):
    assert np.all(np.isneginf(g["log_prob"][b, n0:])) and np.all(g["total"][b, n0:] == -1)
    assert np.all(g["duration_class"][b, n0:] == -1) and np.all(g["duration"][b, n0:] == 0)


# ---- 1. small cases --------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("mode", VR.MODES)
def test_small_bit_exact(gpu, mode, N):
    B, Imax, D = 7, 9, 5
    for seed in range(3):
        logits, I, O = f4_cases.random_case(np.random.default_rng(seed), B, Imax, D)
        table = np.arange(D, dtype=np.int32)
        test_mode, allow_skip = mode == "test_mode", mode != "no_skip"
        mt = int(O.max()) + (9 if test_mode else 0)
        g = _run(gpu, logits, table, I, O, mt, N, 0, allow_skip, test_mode, check=True)
        _same(g, NR.dp(logits, table, I, O, mt, 0, allow_skip, test_mode, N), seed)


@pytest.mark.parametrize("kind", ["tiny", "tie", "wide"])
def test_enumerated_families(gpu, kind):
    full = short = 0
    for seed, mode in NR.family(kind):
        cs = NR.case(kind, seed, mode)
        logits, table, I, O, mt, allow_skip, test_mode = cs
        for N in (2, 8):
            g = _run(gpu, logits, table, I, O, mt, N, 0, allow_skip, test_mode, check=True)
            c = np.array(NR.check_against_paths(g, cs, NR.case_paths(kind, seed, mode), N))
            _same(g, NR.dp(logits, table, I, O, mt, 0, allow_skip, test_mode, N), (kind, seed, mode, N))
        full += int((c >= 8).sum())
        short += int(((c >= 1) & (c <= 7)).sum())
    assert full >= 50 and short >= 10, (kind, full, short)  # full lists and absent ranks both occur


# ---- 2. N = 1 is v2_viterbi_align ------------------------------------------------------------
def _same_as_viterbi(gpu, logits, table, I, O, mt, allow_skip, test_mode):
    args = (_t(np.asarray(logits, np.float32)), _t(table, torch.int32), _t(I, torch.int32), _t(O, torch.int32), 0)
    kw = dict(allow_skip=allow_skip, test_mode=test_mode, max_total=mt)
    v = {k: t.cpu().numpy() for k, t in gpu.v2_viterbi_align(*args, **kw).items()}
    n = {k: t.cpu().numpy() for k, t in gpu.v2_nbest_align(*args, 1, **kw).items()}
    assert n["log_prob"][:, 0].tobytes() == v["log_prob"].tobytes()  # bit for bit, a NaN's too
    for k in KEYS:
        assert np.array_equal(n[k][:, 0], v[k]), k
    assert np.array_equal(n["count"], (v["log_prob"] > -np.inf).astype(np.int32))
    assert int(n["status"][0]) == int(v["status"][0])
    return n


@pytest.mark.parametrize("test_mode", [False, True])
def test_one_best_is_the_viterbi_path(gpu, oracle, test_mode):
    logits, table, I, O, mt = _medium(oracle, test_mode)
    n = _same_as_viterbi(gpu, logits, table, I, O, mt, True, test_mode)
    assert np.all(n["log_prob"] > -np.inf)


def test_one_best_is_the_viterbi_path_on_edge_inputs(gpu):
    logits, table, I, O = _edge_inputs()  # NaN, +inf, all -inf, O > max_total, I = 0, overrun
    n = _same_as_viterbi(gpu, logits, table, I, O, 18, True, False)
    for b in (0, 1, 3, 5):
        _check_absent(n, b)
    assert np.all(n["log_prob"][[2, 6]] > -np.inf)
    for N in (2, 8):  # wider lists: values unspecified on these inputs, the run and the rules are not
        g = _run(gpu, logits, table, I, O, 18, N, check=True)
        for b in (0, 1, 3, 5):
            _check_absent(g, b)


# ---- 3. a rank does not depend on the list width ---------------------------------------------
@functools.lru_cache(maxsize=None)
def _medium_dp(oracle, test_mode, N):
    logits, table, I, O, mt = _medium(oracle, test_mode)
    return NR.dp(logits, table, I, O, mt, 0, True, test_mode, N)


@pytest.mark.parametrize("test_mode", [False, True])
def test_rank_does_not_depend_on_the_list_width(gpu, oracle, test_mode):
    logits, table, I, O, mt = _medium(oracle, test_mode)
    g = {N: _run(gpu, logits, table, I, O, mt, N, 0, True, test_mode, check=True) for N in (3, 4, 5, 8)}
    _same(g[8], _medium_dp(oracle, test_mode, 8))
    assert np.all(g[8]["count"] == 8)
    for small, big in ((3, 4), (3, 8), (5, 8)):
        _same(g[small], _first(g[big], small), (small, big))


# ---- 4. duration tables: both cell forms, every class padding, the rolled class loop ----------
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
    # test mode: rows of 8 ranks must fit LDS, so the totals stop at 600 (paths above it leave the lattice)
    mt = 600 if test_mode else int(O[:4].max())
    if test_mode:
        O = np.minimum(O, mt).astype(np.int32)
    for N in ((4, 8) if D == 40 else (4,)):
        g = _run(gpu, logits, table, I, O, mt, N, 0, True, test_mode, check=True)
        _same(g, NR.dp(logits, table, I, O, mt, 0, True, test_mode, N), (name, N))
        assert np.isfinite(g["log_prob"][:4]).any()


# ---- 5. more than one cell per thread ---------------------------------------------------------
@pytest.mark.parametrize("N", [2, 8])
def test_rows_beyond_one_cell_per_thread(gpu, N):
    B, T, D, mt = 3, 60, 16, 700  # the rows exceed 512 cells from r = 35
    table = np.arange(D, dtype=np.int32)
    logits = _softmax_logits(np.random.default_rng(60 + N), (B, T, D))
    I, O = np.array([T, T - 1, 40], np.int32), np.array([mt, 600, 450], np.int32)
    g = _run(gpu, logits, table, I, O, mt, N, 0, True, True, check=True)
    _same(g, NR.dp(logits, table, I, O, mt, 0, True, True, N))
    assert np.all(g["count"] == N)


# ---- 6. absent ranks --------------------------------------------------------------------------
def test_absent_ranks(gpu):
    logits = np.log(np.array([[[0.5, 0.3, 0.2]], [[0.2, 0.3, 0.5]], [[0.3, 0.3, 0.4]]], np.float32))
    table = np.array([0, 1, 2], np.int32)
    I, O = np.array([1, 1, 2], np.int32), np.array([2, 2, 2], np.int32)  # the last: I > max_steps
    for allow_skip, count in ((True, 3), (False, 2)):
        g = _run(gpu, logits, table, I, O, 2, 8, 0, allow_skip, True)
        _same(g, NR.dp(logits, table, I, O, 2, 0, allow_skip, True, 8), allow_skip)
        assert g["count"].tolist() == [count, count, 0]
        for b in (0, 1):
            assert np.all(g["log_prob"][b, :count] > -np.inf)  # present ranks come first
            _check_absent(g, b, count)
        _check_absent(g, 2)
        assert gpu.load().ssnt_status_from_bits(int(g["status"][0])) == 7  # SSNT_ERR_BAD_LENGTH


# ---- 7. ties ----------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 8])
@pytest.mark.parametrize("test_mode", [False, True])
def test_tie_rich(gpu, test_mode, N):
    B, Imax, D = 8, 40, 6  # the generator of test_gpu_v2_viterbi.py::test_tie_rich
    rng = np.random.default_rng(40 + test_mode)
    table = np.array([0, 3, 4, 3, 5, 4], np.int32)  # two pairs of classes with equal durations
    logits = rng.choice(np.array([-0.5, -1.0, -1.5], np.float32), size=(B, Imax, D))
    logits[0] = -1.0  # one all-equal utterance: every admissible sequence ties
    I = rng.integers(10, Imax + 1, size=B).astype(np.int32)
    I[0] = Imax
    O = np.array([int(rng.integers(3 * i, 5 * i + 1)) for i in I], np.int32)
    mt = int(O.max()) + (5 if test_mode else 0)
    ref = NR.dp(logits, table, I, O, mt, 0, True, test_mode, N)
    assert np.all(ref["count"] == N)
    assert np.all(ref["log_prob"][0] == ref["log_prob"][0, 0])
    _same(_run(gpu, logits, table, I, O, mt, N, 0, True, test_mode, check=True), ref)


# ---- 8. both backpointer stores, both entry widths ---------------------------------------------
def _switch_I(gpu, max_total, test_mode, N):
    """The largest max_steps whose backpointers stay in LDS (by the size query)."""
    q = gpu.load().ssnt_v2_nbest_align_workspace_size
    return switch_point(lambda I: q(1, I, max_total, test_mode, N), hi=1 << 20)


def _poisoned(gpu, logits, table, I, O, mt, test_mode, N):
    """The C entry with a workspace of exactly the queried size in a guarded arena (guarded.py),
    filled with 0xFF, with 0x00, and left as a finished run of other logits of the same shape
    wrote it: the results of the three runs (the guards are checked after each)."""
    lib = gpu.load()
    B, T, D = logits.shape
    need = int(lib.ssnt_v2_nbest_align_workspace_size(B, T, mt, test_mode, N))
    assert need > 0
    f32, i32 = torch.float32, torch.int32
    arena, v = G.lay_out(DEV, {"lg": ((B, T, D), f32), "table": ((D,), i32), "il": ((B,), i32),
                               "ol": ((B,), i32), "log_prob": ((B, N), f32),
                               "duration_class": ((B, N, T), i32), "duration": ((B, N, T), i32),
                               "total": ((B, N), i32), "status": ((1,), i32), "ws": ((need,), torch.uint8)})
    for k, a in (("table", table), ("il", I), ("ol", O)):
        G.put(v[k], np.asarray(a, np.int32))

    def call():
        return G.call(lib, "ssnt_v2_nbest_align_device", v["lg"], v["table"], v["il"], v["ol"], B, T, D,
                      int(mt), 0, True, bool(test_mode), N, v["log_prob"], v["duration_class"], v["duration"],
                      v["total"], v["ws"], need, v["status"], torch.cuda.current_stream().cuda_stream)

    return poisoned_runs(arena, v, lambda x: G.put(v["lg"], np.ascontiguousarray(x, np.float32)), call, logits,
                         logits[::-1, ::-1], OUTS)


@pytest.mark.parametrize("N", [1, 4])
def test_lds_to_workspace_switch(gpu, N):
    mt, test_mode = 300, True
    q = gpu.load().ssnt_v2_nbest_align_workspace_size
    Il = _switch_I(gpu, mt, test_mode, N)
    assert 50 < Il < 1000, Il
    B, D = 2, 8
    table = np.arange(D, dtype=np.int32)
    for T in (Il, Il + 1):
        I, O = np.array([T, T - 40], np.int32), np.array([mt, mt - 5], np.int32)
        logits = _softmax_logits(np.random.default_rng(T), (B, T, D))
        ref = NR.dp(logits, table, I, O, mt, 0, True, test_mode, N)
        assert np.all(ref["count"] == N)
        _same(_run(gpu, logits, table, I, O, mt, N, 0, True, test_mode, check=True), ref, T)
        if q(B, T, mt, test_mode, N) > 0:
            for g in _poisoned(gpu, logits, table, I, O, mt, test_mode, N):
                _same(g, ref, (T, "poisoned"))
    assert q(B, Il, mt, test_mode, N) == 0 and q(B, Il + 1, mt, test_mode, N) > 0


def test_configs4_stores_by_the_size_query(gpu):
    q = gpu.load().ssnt_v2_nbest_align_workspace_size
    assert q(64, 400, 2000, False, 1) == 0 and q(64, 400, 2000, False, 8) > 0
    for N in (1, 2, 4, 8):
        assert q(64, 400, 2000, True, N) > 0  # test mode at the configs[4] shape: the workspace side


@pytest.mark.parametrize("D,N", [(40, 8), (12, 8)], ids=["16-bit entries", "byte entries"])
def test_workspace_entry_widths(gpu, D, N):
    # 64 class slots at list width 8 store 16-bit entries, 16 slots a byte; both in the workspace
    B, T, mt = 2, 120, 100
    assert gpu.load().ssnt_v2_nbest_align_workspace_size(B, T, mt, True, N) > 0
    table = (np.arange(D, dtype=np.int32) * 3) % 11
    logits = _softmax_logits(np.random.default_rng(D), (B, T, D))
    I, O = np.array([T, T - 33], np.int32), np.array([mt, mt - 1], np.int32)
    ref = NR.dp(logits, table, I, O, mt, 0, True, True, N)
    assert np.all(ref["count"] == N)
    _same(_run(gpu, logits, table, I, O, mt, N, 0, True, True, check=True), ref)
    for g in _poisoned(gpu, logits, table, I, O, mt, True, N):
        _same(g, ref, "poisoned")


# ---- 9. the configs[4] row shape, small batch --------------------------------------------------
@functools.lru_cache(maxsize=None)
def _config5_small(oracle, margin=3.0):
    B, I, Ot, D = 4, 400, 2000, 16
    d = oracle.synth_durations(B, I, Ot, D, seed=0)
    logits = oracle.synth_v2_step_logits(d, D, seed=1, margin=margin)
    return logits, np.arange(D, dtype=np.int32), np.full(B, I, np.int32), np.full(B, Ot, np.int32), Ot, d


@pytest.mark.parametrize("test_mode,N", [(False, 8), (True, 4)], ids=["band-8", "test_mode-4"])
def test_config5_rows_bit_exact(gpu, oracle, test_mode, N):
    logits, table, il, ol, Ot, _ = _config5_small(oracle)
    g = _run(gpu, logits, table, il, ol, Ot, N, 0, False, test_mode, check=True)
    _same(g, NR.dp(logits, table, il, ol, Ot, 0, False, test_mode, N))
    assert np.all(g["count"] == N)
    # margin 12: the planted class outweighs every detour, so rank 0 is the planted path (a known
    # answer that does not come from the DP)
    logits, table, il, ol, Ot, d = _config5_small(oracle, 12.0)
    g = _run(gpu, logits, table, il, ol, Ot, N, 0, False, test_mode, check=True)
    assert np.array_equal(g["duration"][:, 0], d) and np.array_equal(g["duration_class"][:, 0], d)
    assert np.all(g["total"][:, 0] == Ot)


# ---- 10. invariants that do not use the DP ---------------------------------------------------
@pytest.mark.parametrize("test_mode", [False, True])
def test_path_invariants(gpu, oracle, test_mode):
    logits, table, I, O, mt = _medium(oracle, test_mode)
    N = 8
    g = _run(gpu, logits, table, I, O, mt, N, 0, True, test_mode, check=True)
    f64 = oracle.v2_fwd_bwd_f64(logits, table, I, O, mt, 0, True, test_mode)["loss"]
    assert np.all(g["count"] == N)
    assert np.all(g["log_prob"][:, 1:] <= g["log_prob"][:, :-1])
    for b in range(len(I)):
        n = int(I[b])
        seen, mass = set(), 0.0
        for k in range(N):
            cls, dur = g["duration_class"][b, k, :n], g["duration"][b, k, :n]
            assert tuple(cls) not in seen, (b, k)
            seen.add(tuple(cls))
            assert np.all(cls >= 0) and np.array_equal(dur, table[cls])
            assert np.all(g["duration_class"][b, k, n:] == -1) and np.all(g["duration"][b, k, n:] == 0)
            assert int(dur.sum()) == int(g["total"][b, k])
            pre = np.cumsum(dur)
            if test_mode:
                assert pre[-1] <= mt
            else:
                assert pre[-1] == O[b]
                for t in range(n):
                    lb, ub = f4_cases.band(t, n, int(O[b]))
                    assert lb <= pre[t] <= ub, (b, k, t)
            v32, v64 = np.float32(0), 0.0
            for t in range(n):
                v32, v64 = np.float32(v32 + logits[b, t, cls[t]]), v64 + float(logits[b, t, cls[t]])
            assert np.float32(v32).tobytes() == g["log_prob"][b, k].tobytes()
            assert v64 <= -f64[b] + 1e-9 * max(1.0, abs(f64[b]))  # one path never outweighs Z
            mass += np.exp(v64 + f64[b])
        assert mass <= 1.0 + 1e-9, (b, mass)  # nor do N distinct ones


# ---- 11. API, error paths, streams -----------------------------------------------------------
def test_need_path_false_and_out_reuse(gpu, oracle):
    logits, table, I, O, mt = _medium(oracle, False)
    B, T, _ = logits.shape
    N = 4
    ref = NR.dp(logits, table, I, O, mt, 0, True, False, N)
    n = _run(gpu, logits, table, I, O, mt, N, need_path=False, check=True)
    assert set(n) == {"log_prob", "count", "status"}
    assert n["log_prob"].tobytes() == ref["log_prob"].tobytes() and np.array_equal(n["count"], ref["count"])
    out = {"log_prob": torch.full((B, N), 7.0, device=DEV),
           "duration_class": torch.full((B, N, T), 9, dtype=torch.int32, device=DEV),
           "duration": torch.full((B, N, T), 9, dtype=torch.int32, device=DEV),
           "total": torch.full((B, N), 9, dtype=torch.int32, device=DEV),
           "status": torch.ones(1, dtype=torch.int32, device=DEV)}
    args = (_t(logits), _t(table), _t(I), _t(O), 0, N)
    r = gpu.v2_nbest_align(*args, allow_skip=True, max_total=mt, out=out, check=True)
    for k in out:
        assert r[k].data_ptr() == out[k].data_ptr()
    _same({k: v.cpu().numpy() for k, v in r.items()}, ref)
    d = gpu.v2_nbest_align(*args, allow_skip=True, check=True)  # max_total defaults to max(O)
    _same({k: v.cpu().numpy() for k, v in d.items()},
          NR.dp(logits, table, I, O, int(O.max()), 0, True, False, N))
    with pytest.raises(ValueError):
        gpu.v2_nbest_align(*args, out={"duration": torch.empty((B, N, T), dtype=torch.int64, device=DEV)})
    with pytest.raises(ValueError):
        gpu.v2_nbest_align(*args, out={"total": torch.empty((B, N + 1), dtype=torch.int32, device=DEV)})
    with pytest.raises(gpu.SsntError):
        gpu.v2_nbest_align(*args[:5], 9)


def test_error_returns_write_nothing(gpu):
    lib = gpu.load()
    B, T, D, mt, N = 2, 6, 4, 12, 8
    x = torch.zeros((B, T, D), device=DEV)
    tb = torch.arange(D, dtype=torch.int32, device=DEV)
    il = torch.full((B,), T, dtype=torch.int32, device=DEV)
    ol = torch.full((B,), mt, dtype=torch.int32, device=DEV)
    lp = torch.full((B, N), 7.0, device=DEV)
    tot = torch.full((B, N), 9, dtype=torch.int32, device=DEV)
    st = torch.zeros(1, dtype=torch.int32, device=DEV)

    def call(lg=x, table=tb, i=il, o=ol, b=B, t=T, d=D, m=mt, test=False, n=N, out=lp, cls=None, ws=None,
             wsb=0):
        return lib.ssnt_v2_nbest_align_device(vp(lg), vp(table), vp(i), vp(o), b, t, d, m, 0, True, test, n,
                                              vp(out), vp(cls), None, vp(tot), vp(ws), wsb, vp(st), None)

    INVALID, UNSUPPORTED, WORKSPACE = 1, 5, 6
    assert call(lg=None) == INVALID and call(table=None) == INVALID and call(i=None) == INVALID
    assert call(o=None) == INVALID and call(out=None) == INVALID
    assert call(b=-1) == INVALID and call(t=0) == INVALID and call(d=0) == INVALID
    assert call(m=-1) == INVALID and call(m=(1 << 24) + 1) == INVALID
    assert call(n=0) == INVALID and call(n=9) == INVALID and call(n=-3) == INVALID
    assert call(d=65) == UNSUPPORTED
    assert call(m=1 << 24, test=True) == UNSUPPORTED  # rows beyond LDS
    assert call(m=4000, test=True, n=8) == UNSUPPORTED  # ... at this list width only (below)
    # a shape whose backpointers need the workspace: missing / one byte short / misaligned
    Tw, mw = 300, 400
    need = int(lib.ssnt_v2_nbest_align_workspace_size(1, Tw, mw, True, N))
    assert need > 0
    big = torch.zeros((1, Tw, D), device=DEV)
    one = torch.full((1,), Tw, dtype=torch.int32, device=DEV)
    cls = torch.full((1, N, Tw), 9, dtype=torch.int32, device=DEV)
    ws = torch.empty(need + 16, dtype=torch.uint8, device=DEV)
    kw = dict(lg=big, i=one, o=one, b=1, t=Tw, m=mw, test=True)
    assert call(cls=cls, **kw) == WORKSPACE
    assert call(cls=cls, ws=ws, wsb=need - 1, **kw) == WORKSPACE
    assert call(cls=cls, ws=ws[1:], wsb=need, **kw) == WORKSPACE
    torch.cuda.synchronize()
    assert torch.all(lp == 7.0) and torch.all(tot == 9) and torch.all(cls == 9)  # a refused call writes nothing
    assert int(st.item()) == 0
    assert call() == 0 and call(m=4000, test=True, n=2) == 0
    assert call(cls=cls, ws=ws, wsb=need, **kw) == 0
    assert call(**kw) == 0  # no path output: no workspace
    assert call(b=0, lg=None, out=None) == 0
    torch.cuda.synchronize()
    assert int(st.item()) == 0 and not torch.any(cls[0, 0] == 9)


def test_bad_length_and_bad_table_status(gpu):
    logits, table, I, O = _edge_inputs()
    logits = np.nan_to_num(logits, nan=-1.0, posinf=-1.0, neginf=-np.inf)  # (finite or -inf: specified values)
    lib = gpu.load()
    N = 4
    I2 = I.copy()
    I2[2] = 7  # > max_steps
    g = _run(gpu, logits, table, I2, O, 18, N)
    _same(g, NR.dp(logits, table, I2, O, 18, 0, True, False, N))
    _check_absent(g, 2)
    assert g["log_prob"][6, 0] > -np.inf
    assert lib.ssnt_status_from_bits(int(g["status"][0])) == 7  # SSNT_ERR_BAD_LENGTH
    with pytest.raises(gpu.SsntError) as e:
        _run(gpu, logits, table, I2, O, 18, N, check=True)
    assert e.value.code == 7
    bad = np.array([0, 1, -2, 3], np.int32)  # a negative entry: every utterance infeasible
    g = _run(gpu, logits, bad, I, O, 18, N)
    _same(g, NR.dp(logits, bad, I, O, 18, 0, True, False, N))
    assert np.all(g["count"] == 0)
    assert lib.ssnt_status_from_bits(int(g["status"][0])) == 8  # SSNT_ERR_BAD_INDEX


def test_two_streams(gpu):
    B, T, D, mt, N = 3, 300, 8, 400, 4  # a workspace shape: each call owns its workspace
    assert gpu.load().ssnt_v2_nbest_align_workspace_size(B, T, mt, True, N) > 0
    table = np.arange(D, dtype=np.int32)
    a = _softmax_logits(np.random.default_rng(1), (B, T, D))
    b = _softmax_logits(np.random.default_rng(2), (B, T, D))
    I, O = np.array([T, T - 9, T - 100], np.int32), np.full(B, mt, np.int32)
    ra, rb = (NR.dp(x, table, I, O, mt, 0, True, True, N) for x in (a, b))
    assert not np.array_equal(ra["duration_class"], rb["duration_class"])
    xa, xb, tb = _t(a), _t(b), _t(table)
    il, ol = _t(I), _t(O)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        ga = gpu.v2_nbest_align(xa, tb, il, ol, 0, N, allow_skip=True, test_mode=True, max_total=mt)
    with torch.cuda.stream(s2):
        gb = gpu.v2_nbest_align(xb, tb, il, ol, 0, N, allow_skip=True, test_mode=True, max_total=mt)
    torch.cuda.synchronize()
    _same({k: v.cpu().numpy() for k, v in ga.items()}, ra, "stream 1")
    _same({k: v.cpu().numpy() for k, v in gb.items()}, rb, "stream 2")
