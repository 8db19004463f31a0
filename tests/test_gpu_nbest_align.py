"""GPU exact N-best alignments (nbest_align.hip) against the numpy-f32 DP of
tests/nbest_ref.py: log_prob, position, duration and count bit / value identical on every lane
layout and list width the envelope admits, ragged extents, 8-byte-aligned inputs, tie-rich and
zero-probability lattices, utterances with fewer than N paths, both backpointer stores (LDS,
workspace); plus checks that use no DP (brute force, the sibling kernels, path invariants), the
input contract (dead cells, guarded buffers, stale bytes) and the error paths."""
import functools
from math import comb

import numpy as np
import pytest
import torch

import contract_cases as CC
import guarded as G
import nbest_ref as NR
from gpu_util import DEV, switch_point, _t, vp
from test_gpu_viterbi import _lattice, _ragged

pytestmark = pytest.mark.gpu

OUTS = ("log_prob", "position", "duration")
INVALID, UNSUPPORTED, WORKSPACE, BAD_LENGTH = 1, 5, 6, 7


def _run(gpu, lt, S, P, N, lo=None, terminal=True, **kw):
    r = gpu.ssnt_nbest_align(lt if isinstance(lt, torch.Tensor) else _t(lt), _t(np.asarray(S), torch.int32),
                             _t(np.asarray(P), torch.int32), N,
                             None if lo is None else (lo if isinstance(lo, torch.Tensor) else _t(lo)),
                             terminal_emit=terminal, **kw)
    return {k: v.cpu().numpy() for k, v in r.items()}


def _same(g, ref, where=""):
    assert g["log_prob"].dtype == np.float32 and g["position"].dtype == np.int32
    assert g["duration"].dtype == np.int32 and g["count"].dtype == np.int32
    assert g["log_prob"].shape == ref["log_prob"].shape, where
    assert g["log_prob"].tobytes() == ref["log_prob"].tobytes(), (where, g["log_prob"], ref["log_prob"])
    assert np.array_equal(g["position"], ref["position"]), where
    assert np.array_equal(g["duration"], ref["duration"]), where
    assert np.array_equal(g["count"], ref["count"]), where


def _max_n(U):
    return 8 if U <= 256 else 4 if U <= 512 else 2


# ---- 1. tiny exhaustive ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tiny(obs, terminal):
    T, U = 7, 4
    SP = [(S, P) for S in range(0, T + 1) for P in range(0, U + 1)]
    lt, lo = _lattice(len(SP), T, U, 5 + obs, obs)
    brute = [NR.brute_force(lt[b], s, p, None if lo is None else lo[b], terminal) for b, (s, p) in enumerate(SP)]
    return SP, lt, lo, brute


@pytest.mark.parametrize("terminal", [True, False])
@pytest.mark.parametrize("obs", [False, True])
@pytest.mark.parametrize("N", [1, 2, 3, 4, 8])
def test_tiny_exhaustive(gpu, N, obs, terminal):
    SP, lt, lo, brute = _tiny(obs, terminal)
    S, P = [s for s, _ in SP], [p for _, p in SP]
    g = _run(gpu, lt, S, P, N, lo, terminal, check=True)
    _same(g, NR.dp(lt, S, P, N, lo, terminal))
    for b, paths in enumerate(brute):
        assert g["log_prob"][b].tobytes() == NR.top_values(paths, N).tobytes(), SP[b]
        assert g["count"][b] == min(N, sum(1 for v, _ in paths if v > -np.inf)), SP[b]


# ---- 2. lane and K boundaries ----------------------------------------------------------------
WIDTHS = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024]


@pytest.mark.parametrize("U", WIDTHS)
def test_lane_boundaries(gpu, U):
    B, T = 3, U + 5
    lt, lo = _lattice(B, T, U, U, obs=(U % 2 == 1))
    S, P = _ragged(U, T)
    # log_trans offset by one (emit, shift) pair: 8-byte aligned only
    flat = torch.empty(lt.size + 2, dtype=torch.float32, device=DEV)
    flat[2:] = _t(lt).reshape(-1)
    off = flat[2:].view(B, T, U, 2)
    assert off.data_ptr() % 16 == 8
    for N in (_max_n(U), 1):
        ref = NR.dp(lt, S, P, N, lo)
        _same(_run(gpu, lt, S, P, N, lo, check=True), ref, (U, N))
        _same(_run(gpu, off, S, P, N, lo, check=True), ref, (U, N, "offset"))


# ---- 3. the list width the kernel runs does not show ----------------------------------------
def test_rank_does_not_depend_on_list_width(gpu):
    B, T, U = 4, 40, 80
    lt, lo = _lattice(B, T, U, 31, obs=True)
    S, P = [40, 40, 33, 12], [40, 7, 20, 12]
    g = {N: _run(gpu, lt, S, P, N, lo, check=True) for N in (3, 4, 5, 8)}
    for N, big in ((3, 4), (3, 8), (5, 8)):
        for k in OUTS:
            assert CC.same_bits(g[N][k], np.ascontiguousarray(g[big][k][:, :N])), (N, big, k)
    _same(g[3], NR.dp(lt, S, P, 3, lo))
    _same(g[5], NR.dp(lt, S, P, 5, lo))


# ---- 4. tie-rich -----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(8, 40, 17), (4, 200, 130)])
def test_tie_rich(gpu, shape):
    B, T, U = shape
    N = 4
    rng = np.random.default_rng(T)
    lt = rng.choice(np.array([-0.5, -1.0, -1.5], np.float32), size=(B, T, U, 2))
    lt[0] = -1.0  # one all-equal lattice: every path ties
    P = rng.integers(1, U + 1, size=B)
    S = np.array([rng.integers(p, T + 1) for p in P])
    S[0], P[0] = T, U
    S[1], P[1] = T, min(T, U)
    for terminal in (True, False):
        g = _run(gpu, lt, S, P, N, terminal=terminal, check=True)
        _same(g, NR.dp(lt, S, P, N, terminal=terminal), terminal)
        # independently of the DP
        assert np.all(g["log_prob"][:, 1:] <= g["log_prob"][:, :-1])
        for b in range(B):
            rows = [tuple(g["position"][b, n]) for n in range(g["count"][b])]
            assert len(set(rows)) == len(rows), b
            for n in range(g["count"][b]):
                v = NR.path_log_prob_f32(lt[b], None, g["position"][b, n], terminal)
                assert np.float32(v).tobytes() == g["log_prob"][b, n].tobytes(), (b, n)


# ---- 5. fewer than N paths -------------------------------------------------------------------
def test_few_paths(gpu):
    B, T, U, N = 6, 9, 5, 8
    lt, lo = _lattice(B, T, U, 9, obs=True)
    S = [9, 1, 5, 3, 4, 6]
    P = [1, 1, 5, 3, 3, 5]  # P = 1; S = P; S = P + 1 with P = 3 (3 paths), with P = 5 (5 paths)
    for n in (N, 4, 2):
        g = _run(gpu, lt, S, P, n, lo, check=True)
        _same(g, NR.dp(lt, S, P, n, lo), n)
        want = [min(n, comb(s - 1, p - 1)) for s, p in zip(S, P)]
        assert g["count"].tolist() == want, n
        for b in range(B):
            c = want[b]
            assert np.all(np.isneginf(g["log_prob"][b, c:])) and np.all(g["log_prob"][b, :c] > -np.inf)
            assert np.all(g["position"][b, c:] == -1) and np.all(g["duration"][b, c:] == 0)


# ---- 6. zero-probability transitions ---------------------------------------------------------
def test_zero_probability_transitions(gpu):
    B, T, U, N = 64, 12, 5, 4
    rng = np.random.default_rng(0)
    lt, _ = _lattice(B, T, U, 1)
    lt[rng.random((B, T, U, 2)) < 0.2] = -np.inf
    S = rng.integers(5, T + 1, size=B)
    P = np.array([rng.integers(1, min(s, U) + 1) for s in S])
    ref = NR.dp(lt, S, P, N)
    g = _run(gpu, lt, S, P, N, check=True)
    _same(g, ref)
    feasible = int(np.sum(g["count"] >= 1))
    assert B // 4 <= feasible <= 3 * B // 4, feasible
    assert np.any((g["count"] > 0) & (g["count"] < N))
    absent = np.arange(N)[None, :] >= g["count"][:, None]
    assert np.all(np.isneginf(g["log_prob"][absent])) and np.all(g["log_prob"][~absent] > -np.inf)
    assert np.all(g["position"][absent] == -1) and np.all(g["duration"][absent] == 0)


# ---- 7. backpointer storage ------------------------------------------------------------------
def _switch_T(gpu, U, N):
    """The largest T whose backpointers stay in LDS at width U and N ranks (by the size query)."""
    return switch_point(lambda T: gpu.load().ssnt_nbest_align_workspace_size(1, T, U, N))


def _c_call(lib, v, B, T, U, N, ws, wsb, flags=1, paths=True):
    return G.call(lib, "ssnt_nbest_align_device", v["lt"], v.get("lo"), v["sl"], v["pl"], B, T, U, N, flags,
                  v["log_prob"], v["position"] if paths else None, v["duration"] if paths else None, ws, wsb,
                  v["status"], torch.cuda.current_stream().cuda_stream)


def _specs(B, T, U, N, obs, wsb):
    f32, i32 = torch.float32, torch.int32
    s = {"lt": ((B, T, U, 2), f32), "sl": ((B,), i32), "pl": ((B,), i32), "status": ((1,), i32),
         "log_prob": ((B, N), f32), "position": ((B, N, T), i32), "duration": ((B, N, U), i32)}
    if obs:
        s["lo"] = ((B, T, U), f32)
    if wsb:
        s["ws"] = ((wsb,), torch.uint8)
    return s


@pytest.mark.parametrize("U,N", [(80, 8), (300, 4)])
def test_lds_to_workspace_switch(gpu, U, N):
    B = 2
    lib = gpu.load()
    Tl = _switch_T(gpu, U, N)
    assert lib.ssnt_nbest_align_workspace_size(B, Tl, U, N) == 0
    need = int(lib.ssnt_nbest_align_workspace_size(B, Tl + 1, U, N))
    assert need > 0 and need % 8 == 0
    for T in (Tl, Tl + 1):
        lt, _ = _lattice(B, T, U, T)
        S, P = [T, T - 7], [min(U, T - 3), max(1, min(U, T) - 29)]
        ref = NR.dp(lt, S, P, N)
        assert ref["count"].tolist() == [N, N]
        g = _run(gpu, lt, S, P, N, check=True)
        _same(g, ref, T)
        n = _run(gpu, lt, S, P, N, need_path=False, check=True)  # no backpointers, no workspace
        assert set(n) == {"log_prob", "count", "status"}
        assert n["log_prob"].tobytes() == ref["log_prob"].tobytes()
    # T = Tl + 1 through the C entry: a short or misaligned workspace is refused and nothing is
    # written; without path outputs no workspace is needed
    T = Tl + 1
    arena, v = G.lay_out(DEV, _specs(B, T, U, N, False, need + 8))
    G.put(v["lt"], lt)
    G.put(v["sl"], np.asarray(S, np.int32))
    G.put(v["pl"], np.asarray(P, np.int32))
    v["status"].zero_()
    for k in OUTS + ("ws",):
        G.fill_bytes(v[k], 0xFF)
    before = {k: G.get(v[k]) for k in OUTS + ("ws",)}
    assert v["ws"].data_ptr() % 8 == 0
    misaligned = v["ws"][4:]
    for ws, wsb in ((v["ws"], need - 1), (None, 0), (None, need), (misaligned, need)):
        assert _c_call(lib, v, B, T, U, N, ws, wsb) == WORKSPACE
        torch.cuda.synchronize()
        assert all(CC.same_bits(G.get(v[k]), before[k]) for k in before)
        assert int(v["status"].item()) == 0
    assert _c_call(lib, v, B, T, U, N, None, 0, paths=False) == 0
    torch.cuda.synchronize()
    assert G.get(v["log_prob"]).tobytes() == ref["log_prob"].tobytes()
    assert all(CC.same_bits(G.get(v[k]), before[k]) for k in ("position", "duration", "ws"))
    assert _c_call(lib, v, B, T, U, N, v["ws"], need) == 0
    torch.cuda.synchronize()
    arena.check()
    for k in OUTS:
        assert CC.same_bits(G.get(v[k]), ref[k]), k


# ---- 8. against the sibling kernels, no DP involved ------------------------------------------
@pytest.mark.parametrize("shape", [(16, 60, 24, 8), (2, 300, 400, 4)])
def test_against_viterbi_and_samples(gpu, shape):
    B, T, U, N = shape
    lt, lo = _lattice(B, T, U, T + U, obs=(U == 24))
    rng = np.random.default_rng(U)
    P = rng.integers(1, min(T, U) + 1, size=B)
    S = np.array([rng.integers(p, T + 1) for p in P])
    S[0], P[0] = T, min(T, U)
    args = (_t(lt), _t(S, torch.int32), _t(P, torch.int32))
    lo_t = None if lo is None else _t(lo)
    vit = {k: x.cpu().numpy() for k, x in gpu.ssnt_viterbi_align(*args, lo_t, check=True).items()}
    one = _run(gpu, lt, S, P, 1, lo, check=True)
    top = _run(gpu, lt, S, P, N, lo, check=True)
    for g in (one, top):
        assert g["log_prob"][:, 0].tobytes() == vit["log_prob"].tobytes()
        assert np.array_equal(g["position"][:, 0], vit["position"])
        assert np.array_equal(g["duration"][:, 0], vit["duration"])
    smp = {k: x.cpu().numpy() for k, x in
           gpu.ssnt_sample_align(*args, 16, lo_t, generator=torch.Generator(DEV).manual_seed(1)).items()}
    assert np.all(smp["log_prob"] <= top["log_prob"][:, :1])
    for b in range(B):
        rows = {tuple(top["position"][b, n]) for n in range(top["count"][b])}
        for k in range(16):
            if smp["log_prob"][b, k] > top["log_prob"][b, N - 1]:
                assert tuple(smp["position"][b, k]) in rows, (b, k)


# ---- 9. contract -----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 20, 9, 8), (3, 75, 70, 4)])
@pytest.mark.parametrize("terminal", [True, False])
def test_dead_cells_are_never_read_into_a_result(gpu, shape, terminal):
    B, T, U, N = shape
    lt, lo = _lattice(B, T, U, 3 * U, obs=True)
    S, P = _ragged(U, T)
    clean = _run(gpu, lt, S, P, N, lo, terminal, check=True)
    _same(clean, NR.dp(lt, S, P, N, lo, terminal))
    for name, value in list(CC.VALUES.items()) + [("alternating", CC.alternating(B))]:
        dlt, dlo = CC.dirty_lattice(lt, lo, S, P, value, terminal)
        g = _run(gpu, dlt, S, P, N, dlo, terminal, check=True)
        for k in OUTS + ("count",):
            assert CC.same_bits(g[k], clean[k]), (name, k)


@pytest.mark.parametrize("case", ["lds", "workspace"])
def test_guarded_buffers_and_stale_bytes(gpu, case):
    lib = gpu.load()
    B, U, N = 2, 80, 8
    T = _switch_T(gpu, U, N) + 1 if case == "workspace" else 45
    wsb = int(lib.ssnt_nbest_align_workspace_size(B, T, U, N))
    assert (wsb > 0) == (case == "workspace")
    lt, lo = _lattice(B, T, U, T + 1, obs=True)
    S, P = [T, T - 9], [U if U <= T else T, 17]
    ref = NR.dp(lt, S, P, N, lo)
    arena, v = G.lay_out(DEV, _specs(B, T, U, N, True, wsb))
    G.put(v["sl"], np.asarray(S, np.int32))
    G.put(v["pl"], np.asarray(P, np.int32))
    got = []
    for guard, fill, first in ((0xA5, 0xFF, None), (0xFF, 0x00, None), (0xA5, None, lt[::-1])):
        arena.fill_guards(guard)
        for x in ([lt] if first is None else [first, lt]):  # the last run: over another lattice's bytes
            G.put(v["lt"], np.ascontiguousarray(x))
            G.put(v["lo"], lo)
            if fill is not None:
                for k in OUTS + ("ws",):
                    G.fill_bytes(v.get(k), fill)
            v["status"].zero_()
            assert _c_call(lib, v, B, T, U, N, v.get("ws"), wsb) == 0
            torch.cuda.synchronize()
            assert int(v["status"].item()) == 0
            arena.check()
        got.append({k: G.get(v[k]) for k in OUTS})
    for g in got:
        for k in OUTS:
            assert CC.same_bits(g[k], ref[k]), k


# ---- 10. errors ------------------------------------------------------------------------------
def test_error_returns(gpu):
    lib = gpu.load()
    B, T, U, N = 2, 6, 3, 4
    x = torch.zeros((B, T, U, 2), device=DEV)
    s = torch.full((B,), T, dtype=torch.int32, device=DEV)
    p = torch.full((B,), U, dtype=torch.int32, device=DEV)
    lp = torch.full((B, 8), 7.0, device=DEV)
    st = torch.zeros(1, dtype=torch.int32, device=DEV)

    def call(lt=x, sl=s, pl=p, b=B, t=T, u=U, n=N, flags=1, out=lp):
        return lib.ssnt_nbest_align_device(vp(lt), None, vp(sl), vp(pl), b, t, u, n, flags, vp(out), None, None,
                                           None, 0, vp(st), None)

    assert call() == 0
    torch.cuda.synchronize()
    lp.fill_(7.0)
    assert call(n=0) == INVALID and call(n=9) == INVALID and call(n=-1) == INVALID
    assert call(flags=2) == INVALID and call(flags=3) == INVALID
    assert call(lt=None) == INVALID and call(sl=None) == INVALID
    assert call(pl=None) == INVALID and call(out=None) == INVALID
    assert call(b=-1) == INVALID and call(t=-1) == INVALID and call(u=-1) == INVALID
    assert call(u=1025, n=1) == UNSUPPORTED and call(u=1025) == UNSUPPORTED
    assert call(u=600, n=4) == UNSUPPORTED and call(u=600, n=3) == UNSUPPORTED
    assert call(u=257, n=8) == UNSUPPORTED and call(u=257, n=5) == UNSUPPORTED
    assert call(b=0, lt=None, out=None) == 0 and call(b=0, n=8) == 0
    torch.cuda.synchronize()
    assert bool(torch.all(lp == 7.0)) and int(st.item()) == 0  # a refused call writes nothing
    for n in (0, 9):
        with pytest.raises(gpu.SsntError) as e:
            gpu.ssnt_nbest_align(x, s, p, n)
        assert e.value.code == INVALID
    with pytest.raises(gpu.SsntError) as e:
        gpu.ssnt_nbest_align(torch.zeros((1, 4, 600, 2), device=DEV), s[:1], p[:1], 4)
    assert e.value.code == UNSUPPORTED
    # the envelope's edges are inside it
    q = lib.ssnt_nbest_align_workspace_size
    assert q(2, 2000, 256, 8) > 0 and q(2, 2000, 512, 4) > 0 and q(2, 2000, 1024, 2) > 0
    assert q(2, 2000, 257, 8) == 0 and q(2, 2000, 80, 9) == 0 and q(0, 2000, 80, 8) == 0


def test_bad_length_status(gpu):
    B, T, U, N = 4, 10, 4, 4
    lt, _ = _lattice(B, T, U, 8)
    S, P = [10, 11, 8, 10], [4, 4, 5, 2]  # [1]: S > T, [2]: P > U
    ref = NR.dp(lt, S, P, N)
    assert ref["count"].tolist() == [4, 0, 0, 4]
    g = _run(gpu, lt, S, P, N)
    _same(g, ref)
    assert gpu.load().ssnt_status_from_bits(int(g["status"][0])) == BAD_LENGTH
    with pytest.raises(gpu.SsntError) as e:
        _run(gpu, lt, S, P, N, check=True)
    assert e.value.code == BAD_LENGTH


@pytest.mark.parametrize("N", [1, 4, 8])
def test_nan_and_inf_inputs_stay_in_bounds(gpu, N):
    B, T, U = 2, 9, 5
    rng = np.random.default_rng(N)
    lt, lo = _lattice(B, T, U, 21, obs=True)
    lt[0][rng.random((T, U, 2)) < 0.3] = np.nan
    lo[0][rng.random((T, U)) < 0.2] = np.nan
    lt[1][rng.random((T, U, 2)) < 0.3] = np.inf
    lt[1][rng.random((T, U, 2)) < 0.2] = -np.inf
    for S, P in (([9, 9], [5, 5]), ([9, 7], [2, 4])):
        g = _run(gpu, lt, S, P, N, lo)  # the call returns; values are unspecified
        assert np.all(g["position"] >= -1) and np.all(g["position"] < U)
        assert np.all(g["duration"] >= 0) and np.all(g["duration"] <= T)


def test_out_reuse(gpu):
    B, T, U, N = 3, 30, 70, 3
    lt, lo = _lattice(B, T, U, 12, obs=True)
    S, P = [30, 22, 30], [30, 20, 1]
    out = {"log_prob": torch.full((B, N), 7.0, device=DEV),
           "position": torch.full((B, N, T), 9, dtype=torch.int32, device=DEV),
           "duration": torch.full((B, N, U), 9, dtype=torch.int32, device=DEV),
           "status": torch.ones(1, dtype=torch.int32, device=DEV)}
    r = gpu.ssnt_nbest_align(_t(lt), _t(np.asarray(S), torch.int32), _t(np.asarray(P), torch.int32), N, _t(lo),
                             out=out, check=True)
    for k in out:
        assert r[k].data_ptr() == out[k].data_ptr()
    _same({k: v.cpu().numpy() for k, v in r.items()}, NR.dp(lt, S, P, N, lo))
    with pytest.raises(ValueError):
        gpu.ssnt_nbest_align(_t(lt), _t(np.asarray(S), torch.int32), _t(np.asarray(P), torch.int32), N,
                             out={"position": torch.empty((B, N + 1, T), dtype=torch.int32, device=DEV)})
