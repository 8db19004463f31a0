"""GPU best-path (Viterbi) alignment (viterbi.hip) against the numpy-f32 DP
of tests/viterbi_ref.py: log_prob, position and duration bit / value identical (np.array_equal)
on every lane layout (K = 1, 2, 4, 8, 16), ragged extents, 8-byte-aligned inputs, tie-rich and
zero-probability lattices, both backpointer stores (LDS, workspace), plus invariants that do not
use the DP, the round trip through upsample_source_indexes, and the error paths."""
import numpy as np
import pytest
import torch

import guarded as G
import lattice_ref
import viterbi_ref as VR
from gpu_util import DEV, poisoned_runs, switch_point, _t, vp

pytestmark = pytest.mark.gpu


def _run(gpu, lt, S, P, lo=None, terminal=True, **kw):
    r = gpu.ssnt_viterbi_align(lt if isinstance(lt, torch.Tensor) else _t(lt), _t(np.asarray(S), torch.int32),
                               _t(np.asarray(P), torch.int32),
                               None if lo is None else (lo if isinstance(lo, torch.Tensor) else _t(lo)),
                               terminal_emit=terminal, **kw)
    return {k: v.cpu().numpy() for k, v in r.items()}


def _same(g, ref, where=""):
    assert g["log_prob"].dtype == np.float32 and g["position"].dtype == np.int32
    assert g["log_prob"].tobytes() == ref["log_prob"].tobytes(), (where, g["log_prob"], ref["log_prob"])
    assert np.array_equal(g["position"], ref["position"]), where
    assert np.array_equal(g["duration"], ref["duration"]), where


def _lattice(B, T, U, seed, obs=False):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((B, T, U, 2)).astype(np.float32) * np.float32(1.5)
    lt = (z - np.logaddexp(z[..., :1], z[..., 1:])).astype(np.float32)
    lo = (rng.standard_normal((B, T, U)) * 3 - 2).astype(np.float32) if obs else None
    return lt, lo


# ---- 1. tiny exhaustive ----------------------------------------------------------------------
@pytest.mark.parametrize("terminal", [True, False])
@pytest.mark.parametrize("obs", [False, True])
def test_tiny_exhaustive(gpu, obs, terminal):
    T, U = 7, 4
    SP = [(S, P) for S in range(0, T + 1) for P in range(0, U + 1)]
    B = len(SP)
    lt, lo = _lattice(B, T, U, 5 + obs, obs)
    S, P = [s for s, _ in SP], [p for _, p in SP]
    ref = VR.dp(lt, S, P, lo, terminal)
    g = _run(gpu, lt, S, P, lo, terminal, check=True)
    _same(g, ref)
    for b, (s, p) in enumerate(SP):
        best, arg = VR.brute_force(lt[b], s, p, None if lo is None else lo[b], terminal)
        assert g["log_prob"][b].tobytes() == np.float32(best).tobytes(), (s, p)
        if arg:
            assert len(arg) == 1 and tuple(g["position"][b, :s]) == arg[0], (s, p)
        else:
            assert np.all(g["position"][b] == -1) and np.all(g["duration"][b] == 0)


# ---- 2. lane / wave / K boundaries -----------------------------------------------------------
# the issue's list plus this kernel's dispatch boundaries (K changes after U = 64, 128, 256, 512)
# and the loaders' rows-per-chunk boundaries (U = 128, 256, 384, 512), each +- 1
WIDTHS = [1, 2, 63, 64, 65, 80, 81, 127, 128, 129, 255, 256, 257, 300, 383, 384, 385, 511, 512,
          513, 1023, 1024]


def _ragged(U, T):
    return [T, T - 2, max(1, T - 4)], [U, 1, max(1, (2 * U) // 3)]


@pytest.mark.parametrize("U", WIDTHS)
def test_lane_boundaries(gpu, U):
    B, T = 3, U + 5
    lt, lo = _lattice(B, T, U, U, obs=(U % 2 == 1))
    S, P = _ragged(U, T)
    ref = VR.dp(lt, S, P, lo)
    _same(_run(gpu, lt, S, P, lo, check=True), ref, U)
    # log_trans offset by one (emit, shift) pair: 8-byte aligned only
    flat = torch.empty(lt.size + 2, dtype=torch.float32, device=DEV)
    flat[2:] = _t(lt).reshape(-1)
    off = flat[2:].view(B, T, U, 2)
    assert off.data_ptr() % 16 == 8
    _same(_run(gpu, off, S, P, lo, check=True), ref, (U, "offset"))


# ---- 3. tie-rich -----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(8, 40, 17), (4, 200, 130)])
def test_tie_rich(gpu, shape):
    B, T, U = shape
    rng = np.random.default_rng(T)
    lt = rng.choice(np.array([-0.5, -1.0, -1.5], np.float32), size=(B, T, U, 2))
    lt[0] = -1.0  # one all-equal lattice: every path ties
    P = rng.integers(1, U + 1, size=B)
    S = np.array([rng.integers(p, T + 1) for p in P])
    S[0], P[0] = T, U
    S[1], P[1] = T, min(T, U)
    _same(_run(gpu, lt, S, P, check=True), VR.dp(lt, S, P))
    _same(_run(gpu, lt, S, P, terminal=False, check=True), VR.dp(lt, S, P, terminal=False))


# ---- 4. zero-probability transitions ---------------------------------------------------------
def test_zero_probability_transitions(gpu):
    B, T, U = 64, 12, 5
    rng = np.random.default_rng(0)
    lt, _ = _lattice(B, T, U, 1)
    lt[rng.random((B, T, U, 2)) < 0.2] = -np.inf
    S = rng.integers(5, T + 1, size=B)
    P = np.array([rng.integers(1, min(s, U) + 1) for s in S])
    ref = VR.dp(lt, S, P)
    feasible = int(np.sum(ref["log_prob"] > -np.inf))
    assert 16 <= feasible <= 48, feasible
    g = _run(gpu, lt, S, P, check=True)
    _same(g, ref)
    bad = ~(g["log_prob"] > -np.inf)
    assert np.all(np.isneginf(g["log_prob"][bad]))
    assert np.all(g["position"][bad] == -1) and np.all(g["duration"][bad] == 0)


# ---- 5. backpointer storage ------------------------------------------------------------------
def _switch_T(gpu, U):
    """The largest T whose backpointer bits stay in LDS at width U (by the size query)."""
    return switch_point(lambda T: gpu.load().ssnt_viterbi_align_workspace_size(1, T, U))


def _poisoned(gpu, lt, S, P):
    """The C entry with a workspace of exactly the queried size in a guarded arena (guarded.py),
    filled with 0xFF, with 0x00, and left as a finished run of another lattice of the same shape
    wrote it: the results of the three runs (the guards are checked after each)."""
    lib = gpu.load()
    B, T, U, _ = lt.shape
    need = int(lib.ssnt_viterbi_align_workspace_size(B, T, U))
    assert need > 0
    f32, i32 = torch.float32, torch.int32
    arena, v = G.lay_out(DEV, {"lt": ((B, T, U, 2), f32), "sl": ((B,), i32), "pl": ((B,), i32),
                               "log_prob": ((B,), f32), "position": ((B, T), i32), "duration": ((B, U), i32),
                               "status": ((1,), i32), "ws": ((need,), torch.uint8)})
    G.put(v["sl"], np.asarray(S, np.int32))
    G.put(v["pl"], np.asarray(P, np.int32))

    def call():
        return G.call(lib, "ssnt_viterbi_align_device", v["lt"], None, v["sl"], v["pl"], B, T, U, 1,
                      v["log_prob"], v["position"], v["duration"], v["ws"], need, v["status"],
                      torch.cuda.current_stream().cuda_stream)

    return poisoned_runs(arena, v, lambda x: G.put(v["lt"], np.ascontiguousarray(x)), call, lt, lt[::-1, ::-1],
                         ("log_prob", "position", "duration"))


@pytest.mark.parametrize("U", [130, 400])
def test_lds_to_workspace_switch(gpu, U):
    B = 2
    Tl = _switch_T(gpu, U)
    lib = gpu.load()
    for T in (Tl, Tl + 1):
        lt, _ = _lattice(B, T, U, T)
        S, P = [T, T - 70], [U, U - 29]
        ref = VR.dp(lt, S, P)
        _same(_run(gpu, lt, S, P, check=True), ref, T)
        if lib.ssnt_viterbi_align_workspace_size(B, T, U) > 0:
            for g in _poisoned(gpu, lt, S, P):
                _same(g, ref, (T, "poisoned"))
    assert lib.ssnt_viterbi_align_workspace_size(B, Tl, U) == 0
    assert lib.ssnt_viterbi_align_workspace_size(B, Tl + 1, U) > 0


@pytest.mark.parametrize("shape", [(2, 2000, 400), (2, 1100, 1024)])
def test_long_shapes(gpu, shape):
    B, T, U = shape
    lt, _ = _lattice(B, T, U, T + U)
    S, P = [T, T - 37], [U, U - 11]
    ref = VR.dp(lt, S, P)
    _same(_run(gpu, lt, S, P, check=True), ref)
    for g in _poisoned(gpu, lt, S, P):
        _same(g, ref, "poisoned")


# ---- 6. headline shape -----------------------------------------------------------------------
def test_headline_shape(gpu, oracle):
    B, T, U = 256, 200, 80  # BASELINE configs[1], the generator and lengths of test_gpu_fwd_bwd.py
    lt = oracle.synth_log_trans(B, T, U, seed=0)
    S, P = [T] * B, [U] * B
    _same(_run(gpu, lt, S, P, check=True), VR.dp(lt, S, P))


# ---- 7. invariants that do not use the DP ----------------------------------------------------
@pytest.mark.parametrize("obs", [False, True])
def test_path_invariants(gpu, obs):
    B, T, U = 4, 30, 9
    lt, lo = _lattice(B, T, U, 77, obs)
    S, P = [30, 25, 9, 17], [9, 4, 9, 1]
    g = _run(gpu, lt, S, P, lo, check=True)
    for b in range(B):
        pos = g["position"][b, :S[b]]
        assert pos[0] == 0 and pos[-1] == P[b] - 1
        assert set(np.diff(pos).tolist()) <= {0, 1}
        assert np.all(g["position"][b, S[b]:] == -1)
        assert np.array_equal(np.bincount(pos, minlength=U), g["duration"][b])
        v32 = lo[b, 0, 0] if obs else np.float32(0)
        v64 = float(v32)
        for s in range(1, S[b]):
            x = lt[b, s - 1, pos[s - 1], int(pos[s] != pos[s - 1])]
            v32, v64 = np.float32(v32 + x), v64 + float(x)
            if obs:
                v32, v64 = np.float32(v32 + lo[b, s, pos[s]]), v64 + float(lo[b, s, pos[s]])
        x = lt[b, S[b] - 1, P[b] - 1, 0]
        v32, v64 = np.float32(v32 + x), v64 + float(x)
        assert np.float32(v32).tobytes() == g["log_prob"][b].tobytes()
        loss, _, _ = lattice_ref.torch_dp(lt[b], S[b], P[b], None if lo is None else lo[b])
        assert v64 <= -loss + 1e-9  # one path's mass is at most log Z


# ---- 8. round trip through upsample_source_indexes --------------------------------------------
def test_round_trip_through_upsample(gpu):
    B, T, U = 6, 50, 21
    lt, _ = _lattice(B, T, U, 3)
    S = np.array([50, 44, 21, 30, 50, 35])
    P = np.array([21, 10, 21, 1, 7, 19])
    r = gpu.ssnt_viterbi_align(_t(lt), _t(S, torch.int32), _t(P, torch.int32), check=True)
    assert bool(torch.all(r["log_prob"] > -np.inf))
    up = gpu.upsample_source_indexes(r["duration"][:, None, :], _t(S, torch.int32)[:, None], -1, 1)[:, 0]
    assert torch.equal(up, r["position"][:, :int(S.max())])


# ---- 9. error paths and stream safety --------------------------------------------------------
def test_error_returns(gpu):
    lib = gpu.load()
    B, T, U = 2, 6, 3
    x = torch.zeros((B, T, U, 2), device=DEV)
    s = torch.full((B,), T, dtype=torch.int32, device=DEV)
    p = torch.full((B,), U, dtype=torch.int32, device=DEV)
    lp = torch.empty(B, device=DEV)
    st = torch.zeros(1, dtype=torch.int32, device=DEV)

    def call(lt=x, sl=s, pl=p, b=B, t=T, u=U, flags=1, out=lp, ws=None, wsb=0, pos=None):
        return lib.ssnt_viterbi_align_device(vp(lt), None, vp(sl), vp(pl), b, t, u, flags, vp(out),
                                             vp(pos), None, vp(ws), wsb, vp(st), None)

    INVALID, UNSUPPORTED, WORKSPACE = 1, 5, 6
    assert call() == 0
    assert call(flags=2) == INVALID and call(flags=3) == INVALID
    assert call(lt=None) == INVALID and call(sl=None) == INVALID
    assert call(pl=None) == INVALID and call(out=None) == INVALID
    assert call(b=-1) == INVALID and call(t=-1) == INVALID and call(u=-1) == INVALID
    assert call(u=1025) == UNSUPPORTED
    assert call(b=0, lt=None, out=None) == 0
    # a shape whose bits need the workspace: missing / too small; not needed without a path
    Tw, Uw = 1100, 1024
    need = int(lib.ssnt_viterbi_align_workspace_size(1, Tw, Uw))
    assert need > 0
    big = torch.zeros((1, Tw, Uw, 2), device=DEV)
    one = torch.ones(1, dtype=torch.int32, device=DEV)
    pos = torch.empty((1, Tw), dtype=torch.int32, device=DEV)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    kw = dict(lt=big, sl=one, pl=one, b=1, t=Tw, u=Uw)
    assert call(pos=pos, **kw) == WORKSPACE
    assert call(pos=pos, ws=ws, wsb=need - 1, **kw) == WORKSPACE
    assert call(pos=pos, ws=ws, wsb=need, **kw) == 0
    assert call(**kw) == 0
    torch.cuda.synchronize()


def test_bad_length_status(gpu):
    B, T, U = 4, 10, 4
    lt, _ = _lattice(B, T, U, 8)
    S, P = [10, 11, 8, 10], [4, 4, 5, 2]  # [1]: S > T, [2]: P > U
    ref = VR.dp(lt, S, P)
    g = _run(gpu, lt, S, P)
    _same(g, ref)
    assert int(g["status"][0]) != 0
    assert gpu.load().ssnt_status_from_bits(int(g["status"][0])) == 7  # SSNT_ERR_BAD_LENGTH
    with pytest.raises(gpu.SsntError) as e:
        _run(gpu, lt, S, P, check=True)
    assert e.value.code == 7


def test_need_path_false_and_out_reuse(gpu):
    B, T, U = 5, 40, 70
    lt, lo = _lattice(B, T, U, 12, obs=True)
    S, P = [40, 33, 40, 12, 25], [40, 20, 1, 12, 25]
    ref = VR.dp(lt, S, P, lo)
    g = _run(gpu, lt, S, P, lo, check=True)
    _same(g, ref)
    n = _run(gpu, lt, S, P, lo, need_path=False, check=True)
    assert set(n) == {"log_prob", "status"}
    assert n["log_prob"].tobytes() == ref["log_prob"].tobytes()
    out = {"log_prob": torch.full((B,), 7.0, device=DEV),
           "position": torch.full((B, T), 9, dtype=torch.int32, device=DEV),
           "duration": torch.full((B, U), 9, dtype=torch.int32, device=DEV),
           "status": torch.ones(1, dtype=torch.int32, device=DEV)}
    r = gpu.ssnt_viterbi_align(_t(lt), _t(np.asarray(S), torch.int32), _t(np.asarray(P), torch.int32),
                               _t(lo), out=out, check=True)
    for k in out:
        assert r[k].data_ptr() == out[k].data_ptr()
    _same({k: v.cpu().numpy() for k, v in r.items()}, ref)
    with pytest.raises(ValueError):
        gpu.ssnt_viterbi_align(_t(lt), _t(np.asarray(S), torch.int32), _t(np.asarray(P), torch.int32),
                               out={"position": torch.empty((B, T), dtype=torch.int64, device=DEV)})
    with pytest.raises(ValueError):
        gpu.ssnt_viterbi_align(_t(lt), _t(np.asarray(S), torch.int32), _t(np.asarray(P), torch.int32),
                               out={"duration": torch.empty((B, U + 1), dtype=torch.int32, device=DEV)})


def test_two_streams(gpu):
    B, T, U = 4, 1000, 400  # a workspace shape: each call owns its workspace
    assert gpu.load().ssnt_viterbi_align_workspace_size(B, T, U) > 0
    a, _ = _lattice(B, T, U, 1)
    b, _ = _lattice(B, T, U, 2)
    S, P = [T] * B, [min(T, U)] * B
    ra, rb = VR.dp(a, S, P), VR.dp(b, S, P)
    assert not np.array_equal(ra["position"], rb["position"])
    xa, xb = _t(a), _t(b)
    s, p = _t(np.asarray(S), torch.int32), _t(np.asarray(P), torch.int32)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        ga = gpu.ssnt_viterbi_align(xa, s, p)
    with torch.cuda.stream(s2):
        gb = gpu.ssnt_viterbi_align(xb, s, p)
    torch.cuda.synchronize()
    _same({k: v.cpu().numpy() for k, v in ga.items()}, ra, "stream 1")
    _same({k: v.cpu().numpy() for k, v in gb.items()}, rb, "stream 2")
