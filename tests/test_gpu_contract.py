"""A lattice call's outputs are a function of exactly the bytes its contract names, and it writes
exactly the bytes its contract names (DESIGN.md 6 "Contract tests").

Every tensor of a call lives in one guarded arena (tests/guarded.py); the workspace and the sum
state are exactly as long as the entry's query says. The reference is computed once, from the
clean input. The entry then runs three times:

  run  dead input cells                      guards  workspace before      outputs before
  A    clean                                 0xA5    0x00                  0xFF
  B    all-ones NaN                          0xFF    0xFF                  0x5A
  C    +inf / 1e30 / 88 by utterance         0xA5    left by a finished run of a different input
                                                     of the same shape, as are the outputs

After each run: the status word, every output against the reference (with the comparison the
entry's own test file uses), the guards. A, B and C are bit-identical to each other. The input
guards are NaN in B and finite in A and C, so a read outside a tensor that reaches a result shows
as a difference. tests/test_contract_ref.py holds the references to the same dead-cell classes."""
import functools

import numpy as np
import pytest
import torch

import contract_cases as CC
import guarded as G
import sample_cases as SC
import v2_viterbi_ref as V2R
import viterbi_ref as VR
from f4_cases import random_case
from gpu_util import DEV, _t
from loss_sum_ref import wave_order_sum
from test_gpu_fwd_bwd import _assert_bit_exact, _check_debug64
from test_gpu_sample_align import _check as _check_sample
from test_gpu_v2_fwd_bwd import F4_TABLES
from test_gpu_v2_fwd_bwd import _same as _same_v2
from test_gpu_v2_viterbi import _edge_inputs, _softmax_logits, _switch_I
from test_gpu_v2_viterbi import _same as _same_v2_viterbi
from test_gpu_viterbi import _lattice, _ragged, _switch_T
from test_gpu_viterbi import _same as _same_viterbi

pytestmark = pytest.mark.gpu

F32, I32, U8 = torch.float32, torch.int32, torch.uint8
F_TERM, F_ZINF = 1, 2
BAD_LENGTH_BIT = 4  # kStatusBadLength (ssnt_status_from_bits -> SSNT_ERR_BAD_LENGTH = 7)

# (run, guard byte, workspace fill, output fill); "other" is the finished run C's stale bytes are from
RUNS = (("A", 0xA5, 0x00, 0xFF), ("B", 0xFF, 0xFF, 0x5A), ("other", 0xA5, None, None),
        ("C", 0xA5, None, None))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def three_runs(lib, entry, specs, args, inputs, outs, check, status_bits=0, scratch=("ws",)):
    """specs: the arena's blocks; args(v): the entry's argument list from the views; inputs[run]:
    name -> array for the runs A, B, other, C; outs: the output blocks; check(got, run) compares one
    run's outputs with the reference. Returns A's outputs."""
    arena, v = G.lay_out(DEV, specs)
    got = {}
    for run, guard, ws_fill, out_fill in RUNS:
        arena.fill_guards(guard)
        for k, a in inputs[run].items():
            G.put(v[k], a)
        if ws_fill is not None:
            for k in scratch:
                G.fill_bytes(v.get(k), ws_fill)
        if out_fill is not None:
            for k in outs:
                G.fill_bytes(v[k], out_fill)
        v["status"].zero_()
        assert G.call(lib, entry, *args(v)) == 0, (entry, run)
        torch.cuda.synchronize()
        assert int(v["status"].item()) == status_bits, (entry, run)
        arena.check()
        got[run] = {k: G.get(v[k]) for k in outs}
        if run != "other":
            try:
                check(got[run], run)
            except AssertionError as e:
                raise AssertionError(f"{entry}, run {run}: {e}") from None
    for run in ("B", "C"):
        for k in outs:
            assert CC.same_bits(got[run][k], got["A"][k]), f"{entry}: {k} of run {run} differs from run A"
    return got["A"]


def _ws_spec(specs, nbytes):
    if nbytes:
        specs["ws"] = ((nbytes,), U8)


# ---- ssnt_fwd_bwd_device ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stream_Ts(U):
    """The largest T the default dispatch keeps in LDS at width U, by the size query (B = 2), as
    test_workspace_query_matches_dispatch_at_lds_boundary finds it."""
    import ssnt_tts_amd
    lib = ssnt_tts_amd.load()
    zero = [T for T in range(1, 331) if lib.ssnt_fwd_bwd_workspace_size(2, T, U) == 0]
    assert zero and len(zero) < 330
    return max(zero)


def _edge_lengths(seed, B, T, U):
    rng = np.random.default_rng(seed)  # the lengths of test_bit_exact_ragged_and_edges
    P = rng.integers(1, U + 1, size=B)
    S = np.array([rng.integers(max(1, p), T + 1) for p in P])
    S[0], P[0] = 1, 1
    S[1], P[1] = 10, 12
    S[2], P[2] = 0, 1
    S[3], P[3] = T, U
    S[4], P[4] = 20, 20
    return S, P


def _wide_lengths(B, T, U):
    rng = np.random.default_rng(U + T)  # the lengths of test_wide_rows_bit_exact
    P = [min(U, T)] + [int(x) for x in rng.integers(1, min(U, T) + 1, size=B - 1)]
    S = [T] + [int(rng.integers(p, T + 1)) for p in P[1:]]
    return np.array(S), np.array(P)


def _fb_shape(name):
    """(B, T, U, S, P, flags, offset in bytes of log_trans and grad)."""
    if name.startswith("edges"):
        flags = {"edges-f1": F_TERM, "edges-f0": 0, "edges-f3": F_TERM | F_ZINF}[name]
        return (9, 48, 33, *_edge_lengths(0, 9, 48, 33), flags, 0)
    if name == "ragged-65":
        return (4, 60, 65, [60, 41, 33, 7], [60, 40, 17, 1], F_TERM, 0)
    if name == "ragged-130":
        return (3, 45, 130, [45, 44, 30], [45, 13, 30], F_TERM, 0)
    if name == "ws-320x80":
        return (3, 320, 80, [320, 250, 200], [80, 70, 33], F_TERM, 0)
    if name.startswith("ws-U"):
        U = int(name.split("U")[1].split("-")[0])
        T = _stream_Ts(U) + 1
        return (2, T, U, [T, T - 9], [min(U, T), min(U, T - 9) - 5], F_TERM, 4 if name.endswith("-offset") else 0)
    B, T, U = {"long-257": (2, 40, 257), "long-400": (3, 64, 400), "long-512": (2, 36, 512),
               "long-777": (3, 26, 777), "long-1024": (2, 24, 1024)}[name]
    return (B, T, U, *_wide_lengths(B, T, U), F_TERM, 0)


@functools.lru_cache(maxsize=None)
def _fb_case(name, obs):
    """Inputs of the four runs and the oracle's outputs on the clean one."""
    import oracle
    B, T, U, S, P, flags, off = _fb_shape(name)
    S, P = np.asarray(S, np.int32), np.asarray(P, np.int32)
    seed = sum(map(ord, name))
    lt = oracle.synth_log_trans(B, T, U, seed=seed)
    other = oracle.synth_log_trans(B, T, U, seed=seed + 1)
    rng = np.random.default_rng(seed)
    lo = (rng.standard_normal((B, T, U)) * 15 - 40).astype(np.float32) if obs else None
    lo2 = (rng.standard_normal((B, T, U)) * 15 - 40).astype(np.float32) if obs else None
    term = bool(flags & F_TERM)
    ins = {"A": (lt, lo), "B": CC.dirty_lattice(lt, lo, S, P, CC.VALUES["nan_ones"], term),
           "other": (other, lo2), "C": CC.dirty_lattice(lt, lo, S, P, CC.alternating(B), term)}
    inputs = {}
    for run, (x, o) in ins.items():
        inputs[run] = {"lt": x, "sl": S, "pl": P}
        if obs:
            inputs[run]["lo"] = o
    assert not CC.same_bits(inputs["A"]["lt"], inputs["B"]["lt"])
    ref = oracle.fwd_bwd_xf(lt, S, P, log_obs=lo, flags=flags, debug=True)
    return (B, T, U, flags, off), inputs, ref


def _fb_run(lib, name, obs, debug):
    (B, T, U, flags, off), inputs, ref = _fb_case(name, obs)
    specs = {"lt": ((B, T, U, 2), F32, off), "sl": ((B,), I32), "pl": ((B,), I32), "status": ((1,), I32),
             "loss": ((B,), F32), "grad": ((B, T, U, 2), F32, off)}
    outs = ["loss", "grad"]
    if obs:
        specs["lo"], specs["grad_obs"] = ((B, T, U), F32), ((B, T, U), F32)
        outs.append("grad_obs")
    if debug:
        specs["log_alpha"], specs["log_beta"] = ((B, T, U), F32), ((B, T, U), F32)
        outs += ["log_alpha", "log_beta"]
    wsb = int(lib.ssnt_fwd_bwd_workspace_size(B, T, U))
    _ws_spec(specs, wsb)

    def args(v):
        return (v["lt"], v.get("lo"), v["sl"], v["pl"], B, T, U, flags, v["loss"], v["grad"],
                v.get("grad_obs"), v.get("log_alpha"), v.get("log_beta"), v.get("ws"), wsb, v["status"],
                _stream())

    three_runs(lib, "ssnt_fwd_bwd_device", specs, args, inputs, outs,
               lambda g, run: _assert_bit_exact(g, ref, outs))
    return wsb


SMALL = ["edges-f1", "edges-f0", "edges-f3", "ragged-65", "ragged-130", "ws-320x80", "ws-U256", "ws-U81",
         "ws-U81-offset"]
LONG = ["long-257", "long-400", "long-512", "long-777", "long-1024"]


@pytest.mark.parametrize("obs", [False, True], ids=["plain", "obs"])
@pytest.mark.parametrize("variant", [0, 1, 2], ids=["default", "simple", "segmented"])
@pytest.mark.parametrize("name", SMALL)
def test_fwd_bwd(gpu, name, variant, obs):
    for debug in (False, True):
        if variant == 0:
            wsb = _fb_run(gpu.load(), name, obs, debug)
            k = gpu.last_fwd_bwd_kernel()
            if name.startswith("ws-"):
                # the streaming kernel with a workspace (past T* the form with the smaller rings may
                # still keep its rows in LDS; at 320 x 80 no form does)
                assert wsb > 0 and k.startswith("k_fwd_bwd_stream<"), k
                assert name != "ws-320x80" or "LDS=0" in k, k
            continue
        with gpu.use_ab() as ab:
            assert ab.ssnt_fwd_bwd_set_variant(variant) == 0
            _fb_run(ab, name, obs, debug)
            k = gpu.last_fwd_bwd_kernel()
            # (the segmented kernel declines a 4-byte-aligned log_trans: another kernel runs)
            if not name.endswith("-offset"):
                assert k.startswith("k_fwd_bwd_wide<" if variant == 2 else "k_fwd_bwd<"), k


@pytest.mark.parametrize("obs", [False, True], ids=["plain", "obs"])
@pytest.mark.parametrize("name", LONG)
def test_fwd_bwd_long_rows(gpu, name, obs):
    # the default dispatch's long-row kernel with a direction's segments split over two
    # workgroups (global hand-off rings and counters in the workspace) and in one workgroup, and
    # the two-wave kernel where it takes the width
    seen = set()
    with gpu.use_ab() as ab:
        for split in (1, 0):
            assert ab.ssnt_fwd_bwd_wide_split(split) == 0
            for debug in (False, True):
                _fb_run(ab, name, obs, debug)
                k = gpu.last_fwd_bwd_kernel()
                assert k.startswith("k_fwd_bwd_wide<") and ("SPLIT" in k) == bool(split), k
                seen.add("SPLIT" in k)
        assert seen == {True, False}, "a SPLIT instance and a one-workgroup instance both ran"
        ab.ssnt_fwd_bwd_wide_split(-1)
        if _fb_shape(name)[2] <= 512:
            assert ab.ssnt_fwd_bwd_set_variant(1) == 0
            for debug in (False, True):
                _fb_run(ab, name, obs, debug)
                assert gpu.last_fwd_bwd_kernel().startswith("k_fwd_bwd<"), gpu.last_fwd_bwd_kernel()


# ---- ssnt_fwd_bwd_debug64_device --------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 40, 24), (2, 40, 257)])
def test_fwd_bwd_debug64(gpu, oracle, shape):
    lib = gpu.load()
    B, T, U = shape
    S, P = (np.array([40, 31, 24]), np.array([24, 20, 24])) if U == 24 else _wide_lengths(B, T, U)
    S, P = S.astype(np.int32), P.astype(np.int32)
    lt = oracle.synth_log_trans(B, T, U, seed=23)
    inputs = {"A": lt, "B": CC.dirty_lattice(lt, None, S, P, CC.VALUES["nan_ones"], True)[0],
              "other": oracle.synth_log_trans(B, T, U, seed=24),
              "C": CC.dirty_lattice(lt, None, S, P, CC.alternating(B), True)[0]}
    inputs = {run: {"lt": x, "sl": S, "pl": P} for run, x in inputs.items()}
    wsb = int(lib.ssnt_fwd_bwd_debug64_workspace_size(B, T, U))
    assert wsb > 0
    specs = {"lt": ((B, T, U, 2), F32), "sl": ((B,), I32), "pl": ((B,), I32), "status": ((1,), I32),
             "loss": ((B,), torch.float64), "grad": ((B, T, U, 2), F32),
             "log_alpha": ((B, T, U), torch.float64), "log_beta": ((B, T, U), torch.float64),
             "ws": ((wsb,), U8)}
    outs = ["loss", "grad", "log_alpha", "log_beta"]

    def args(v):
        return (v["lt"], None, v["sl"], v["pl"], B, T, U, F_TERM, v["loss"], v["grad"], None,
                v["log_alpha"], v["log_beta"], v["ws"], wsb, v["status"], _stream())

    three_runs(lib, "ssnt_fwd_bwd_debug64_device", specs, args, inputs, outs,
               lambda g, run: _check_debug64(g, lt, S, P, oracle, f64=False))


# ---- ssnt_viterbi_align_device ----------------------------------------------------------------
def _viterbi_case(lt, lo, S, P, seed):
    B, T, U, _ = lt.shape
    S, P = np.asarray(S, np.int32), np.asarray(P, np.int32)
    lt2, lo2 = _lattice(B, T, U, seed + 1000, obs=lo is not None)
    ins = {"A": (lt, lo), "B": CC.dirty_lattice(lt, lo, S, P, CC.VALUES["nan_ones"], True),
           "other": (lt2, lo2), "C": CC.dirty_lattice(lt, lo, S, P, CC.alternating(B), True)}
    inputs = {}
    for run, (x, o) in ins.items():
        inputs[run] = {"lt": x, "sl": S, "pl": P}
        if lo is not None:
            inputs[run]["lo"] = o
    return inputs, VR.dp(lt, S, P, lo)


def _viterbi_run(gpu, lt, lo, S, P, seed):
    lib = gpu.load()
    B, T, U, _ = lt.shape
    inputs, ref = _viterbi_case(lt, lo, S, P, seed)
    specs = {"lt": ((B, T, U, 2), F32), "sl": ((B,), I32), "pl": ((B,), I32), "status": ((1,), I32),
             "log_prob": ((B,), F32), "position": ((B, T), I32), "duration": ((B, U), I32)}
    if lo is not None:
        specs["lo"] = ((B, T, U), F32)
    wsb = int(lib.ssnt_viterbi_align_workspace_size(B, T, U))
    _ws_spec(specs, wsb)

    def args(v):
        return (v["lt"], v.get("lo"), v["sl"], v["pl"], B, T, U, F_TERM, v["log_prob"], v["position"],
                v["duration"], v.get("ws"), wsb, v["status"], _stream())

    three_runs(lib, "ssnt_viterbi_align_device", specs, args, inputs, ["log_prob", "position", "duration"],
               lambda g, run: _same_viterbi(g, ref, run))
    return wsb


@pytest.mark.parametrize("U", [1, 64, 65, 129, 257, 513, 1024])
def test_viterbi_align(gpu, U):
    B, T = 3, U + 5
    lt, lo = _lattice(B, T, U, U, obs=(U % 2 == 1))
    _viterbi_run(gpu, lt, lo, *_ragged(U, T), U)


def test_viterbi_align_workspace_mode(gpu):
    U = 130
    T = _switch_T(gpu, U) + 1
    lt, _ = _lattice(2, T, U, T)
    assert _viterbi_run(gpu, lt, None, [T, T - 70], [U, U - 29], T) > 0


# ---- ssnt_sample_align_device -----------------------------------------------------------------
SAMPLE_CASES = {"reuse": lambda lib: SC.reuse(), "lane65": lambda lib: SC.lane(65),
                "lane257": lambda lib: SC.lane(257), "lane513": lambda lib: SC.lane(513),
                "k64": lambda lib: SC.k_edge(64), "switch": lambda lib: SC.switch(SC.switch_T(lib) + 1)}


@pytest.mark.parametrize("name", list(SAMPLE_CASES))
def test_sample_align(gpu, name):
    lib = gpu.load()
    c = SAMPLE_CASES[name](lib)
    lt, lo, S, P, K, u = c["lt"], c["lo"], c["S"], c["P"], c["K"], c["u"]
    B, T, U, _ = lt.shape
    term = c["terminal"]
    lt2, lo2 = SC.lattice(B, T, U, 4242, obs=lo is not None)
    ins = {"A": (lt, lo, u), "B": (*CC.dirty_lattice(lt, lo, S, P, CC.VALUES["nan_ones"], term), u),
           "other": (lt2, lo2, SC.uniforms(B, K, T, 4242)),
           "C": (*CC.dirty_lattice(lt, lo, S, P, CC.alternating(B), term), u)}
    inputs = {}
    for run, (x, o, un) in ins.items():
        inputs[run] = {"lt": x, "sl": S, "pl": P, "u": un}
        if lo is not None:
            inputs[run]["lo"] = o
    specs = {"lt": ((B, T, U, 2), F32), "sl": ((B,), I32), "pl": ((B,), I32), "u": ((B, K, T), F32),
             "status": ((1,), I32), "log_prob": ((B, K), F32), "position": ((B, K, T), I32),
             "duration": ((B, K, U), I32)}
    if lo is not None:
        specs["lo"] = ((B, T, U), F32)
    wsb = int(lib.ssnt_sample_align_workspace_size(B, T, U, K))
    assert (wsb > 0 or name != "switch") and (wsb == 0 or name != "reuse")  # both decision-bit stores
    _ws_spec(specs, wsb)

    def args(v):
        return (v["lt"], v.get("lo"), v["sl"], v["pl"], v["u"], B, T, U, K, int(term), v["log_prob"],
                v["position"], v["duration"], v.get("ws"), wsb, v["status"], _stream())

    three_runs(lib, "ssnt_sample_align_device", specs, args, inputs, ["log_prob", "position", "duration"],
               lambda g, run: _check_sample(c, g, where=f"{name} run {run}"))


# ---- ssnt_v2_fwd_bwd_device, ssnt_v2_viterbi_align_device -------------------------------------
def _v2_case(name):
    """logits, table, I, O, max_total, allow_skip, test_mode."""
    if name in V2R.MODES:
        logits, I, O = random_case(np.random.default_rng(0), 7, 9, 5)
        test_mode, allow_skip = name == "test_mode", name != "no_skip"
        return logits, np.arange(5, dtype=np.int32), I, O, int(O.max()) + (9 if test_mode else 0), allow_skip, test_mode
    if name == "edges":
        logits, table, I, O = _edge_inputs()
        return logits, table, I, O, 18, True, False
    if name == "viterbi-workspace":  # the smallest workspace-mode case of test_lds_to_workspace_switch
        import ssnt_tts_amd
        mt, D = 300, 8
        T = _switch_I(ssnt_tts_amd, mt, True) + 1
        return (_softmax_logits(np.random.default_rng(T), (2, T, D)), np.arange(D, dtype=np.int32),
                np.array([T, T - 70], np.int32), np.array([mt, mt - 5], np.int32), mt, True, True)
    tname, test_mode = name.rsplit("-", 1)
    test_mode = test_mode == "test"
    table = np.array(dict(F4_TABLES)[tname], np.int32)  # the batch of test_duration_tables_bit_exact
    D, B, Imax = len(table), 5, 150
    rng = np.random.default_rng(D)
    logits = _softmax_logits(rng, (B, Imax, D))
    I = np.array([150, 149, 97, 70, 20], np.int32)
    O = np.array([int(table[rng.integers(0, D, size=i)].sum()) for i in I], np.int32)
    O[4] = int(I[4]) * (int(table.max()) + 30)
    mt = int(O[:4].max()) + (7 if test_mode else 0)
    if test_mode:
        O[4] = min(int(O[4]), mt)
    return logits, table, I, O, mt, True, test_mode


def _v2_inputs(case):
    logits, table, I, O, mt, allow_skip, test_mode = case
    B = logits.shape[0]
    other = _softmax_logits(np.random.default_rng(777), logits.shape)
    lg = {"A": logits, "B": CC.dirty_v2(logits, I, CC.VALUES["nan_ones"], 0, allow_skip), "other": other,
          "C": CC.dirty_v2(logits, I, CC.alternating(B), 0, allow_skip)}
    return {run: {"lg": x, "table": np.asarray(table, np.int32), "il": np.asarray(I, np.int32),
                  "ol": np.asarray(O, np.int32)} for run, x in lg.items()}


V2_CASES = V2R.MODES + ["edges", "long_durations-band", "long_durations-test", "d40-band", "d40-test"]


@pytest.mark.parametrize("name", V2_CASES)
def test_v2_fwd_bwd(gpu, oracle, name):
    lib = gpu.load()
    case = _v2_case(name)
    logits, table, I, O, mt, allow_skip, test_mode = case
    B, T, D = logits.shape
    X = mt + 1
    for flags in ((0, F_ZINF) if name == "edges" else (0,)):
        ref = oracle.v2_fwd_bwd(logits, table, I, O, mt, 0, allow_skip, test_mode, flags=flags, debug=True)
        for debug in (False, True):
            specs = {"lg": ((B, T, D), F32), "table": ((D,), I32), "il": ((B,), I32), "ol": ((B,), I32),
                     "status": ((1,), I32), "loss": ((B,), F32), "grad": ((B, T, D), F32)}
            outs = ["loss", "grad"]
            if debug:
                specs["log_alpha"], specs["log_beta"] = ((B, T + 1, X), F32), ((B, T + 1, X), F32)
                outs += ["log_alpha", "log_beta"]
            wsb = int(lib.ssnt_v2_fwd_bwd_workspace_size(B, T, mt, test_mode))
            _ws_spec(specs, wsb)

            def args(v):
                return (v["lg"], v["table"], v["il"], v["ol"], B, T, D, mt, 0, allow_skip, test_mode, flags,
                        v["loss"], v["grad"], v.get("log_alpha"), v.get("log_beta"), v.get("ws"), wsb,
                        v["status"], _stream())

            three_runs(lib, "ssnt_v2_fwd_bwd_device", specs, args, _v2_inputs(case), outs,
                       lambda g, run: _same_v2(g, ref, outs))


@pytest.mark.parametrize("name", V2_CASES + ["viterbi-workspace"])
def test_v2_viterbi_align(gpu, name):
    lib = gpu.load()
    case = _v2_case(name)
    logits, table, I, O, mt, allow_skip, test_mode = case
    B, T, D = logits.shape
    ref = V2R.dp(logits, table, I, O, mt, 0, allow_skip, test_mode)
    specs = {"lg": ((B, T, D), F32), "table": ((D,), I32), "il": ((B,), I32), "ol": ((B,), I32),
             "status": ((1,), I32), "log_prob": ((B,), F32), "duration_class": ((B, T), I32),
             "duration": ((B, T), I32), "total": ((B,), I32)}
    wsb = int(lib.ssnt_v2_viterbi_align_workspace_size(B, T, mt, test_mode))
    assert wsb > 0 or name != "viterbi-workspace"
    _ws_spec(specs, wsb)

    def args(v):
        return (v["lg"], v["table"], v["il"], v["ol"], B, T, D, mt, 0, allow_skip, test_mode, v["log_prob"],
                v["duration_class"], v["duration"], v["total"], v.get("ws"), wsb, v["status"], _stream())

    three_runs(lib, "ssnt_v2_viterbi_align_device", specs, args, _v2_inputs(case),
               ["log_prob", "duration_class", "duration", "total"],
               lambda g, run: _same_v2_viterbi(g, ref, run))


# ---- the loss-sum state -----------------------------------------------------------------------
def test_loss_sum_state_schedule(gpu, oracle):
    # one state, zeroed once, then left to the library: B shrinking and growing, more workgroups
    # than CUs, a call that reports a bad length, an empty batch, a shape whose sum is a pass of
    # its own, and back
    lib = gpu.load()
    nstate = int(lib.ssnt_fwd_bwd_sum_state_size(600))
    state_arena, sv = G.lay_out(DEV, {"state": ((nstate,), U8)})
    sv["state"].zero_()
    flags = F_TERM | F_ZINF
    schedule = [(70, 24, 16, False), (256, 24, 16, False), (1, 24, 16, False), (600, 24, 16, False),
                (3, 24, 16, True), (0, 24, 16, False), (2, 30, 300, False), (70, 24, 16, False)]
    for step, (B, T, U, bad) in enumerate(schedule):
        Bn = max(B, 1)  # (an empty batch still passes valid pointers)
        rng = np.random.default_rng(100 + step)
        lt = oracle.synth_log_trans(Bn, T, U, seed=100 + step)
        P = rng.integers(1, min(T, U) + 1, size=Bn)
        S = np.array([rng.integers(max(1, p), T + 1) for p in P])
        if bad:
            S[1] = T + 1
        ref = oracle.fwd_bwd_xf(lt, S, P, flags=flags)
        wsb = int(lib.ssnt_fwd_bwd_workspace_size(B, T, U))
        specs = {"lt": ((Bn, T, U, 2), F32), "sl": ((Bn,), I32), "pl": ((Bn,), I32), "status": ((1,), I32),
                 "loss": ((Bn,), F32), "grad": ((Bn, T, U, 2), F32), "loss_sum": ((1,), F32)}
        _ws_spec(specs, wsb)
        arena, v = G.lay_out(DEV, specs)
        G.put(v["lt"], lt)
        G.put(v["sl"], S.astype(np.int32))
        G.put(v["pl"], P.astype(np.int32))
        for k in ("loss", "grad", "loss_sum", "ws"):
            G.fill_bytes(v.get(k), 0xFF)
        v["status"].zero_()
        rc = G.call(lib, "ssnt_fwd_bwd_sum_device", v["lt"], None, v["sl"], v["pl"], B, T, U, flags, v["loss"],
                    v["grad"], None, None, None, v.get("ws"), wsb, v["status"], v["loss_sum"], sv["state"],
                    _stream())
        assert rc == 0, step
        torch.cuda.synchronize()
        where = (step, B, T, U, gpu.last_fwd_bwd_kernel())
        assert int(v["status"].item()) == (BAD_LENGTH_BIT if bad else 0), where
        arena.check()
        state_arena.check()
        got_sum = G.get(v["loss_sum"])
        if B == 0:
            assert got_sum.tobytes() == np.float32([0.0]).tobytes(), where
            assert bool(torch.all(v["loss"].view(-1).view(U8) == 0xFF)), "an empty batch writes no loss"
            continue
        assert ("+k_loss_sum" in gpu.last_fwd_bwd_kernel()) == (U > 256), where
        _assert_bit_exact({"loss": G.get(v["loss"]), "grad": G.get(v["grad"])}, ref, ["loss", "grad"])
        assert got_sum.tobytes() == np.float32([wave_order_sum(ref["loss"])]).tobytes(), (where, got_sum)


# ---- two streams ------------------------------------------------------------------------------
def test_fwd_bwd_two_streams(gpu, oracle):
    # a workspace-mode streaming shape on one stream, a long-row shape on another, each with its
    # own in-launch / separate-pass loss sum (the mirror keeps one sum state per stream), issued
    # twice, interleaved: the serial results
    cases = []
    for (B, T, U), (S, P) in (((3, 320, 80), ([320, 250, 200], [80, 70, 33])),
                              ((2, 40, 257), _wide_lengths(2, 40, 257))):
        lt = oracle.synth_log_trans(B, T, U, seed=U)
        ref = oracle.fwd_bwd_xf(lt, S, P)
        t = (torch.from_numpy(lt).to(DEV), torch.tensor(np.asarray(S), dtype=I32, device=DEV),
             torch.tensor(np.asarray(P), dtype=I32, device=DEV))
        cases.append((t, ref))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    res = []
    for _ in range(2):
        for (t, _), s in zip(cases, streams):
            with torch.cuda.stream(s):
                res.append(gpu.ssnt_fwd_bwd(*t, loss_sum=True, check=False))
    torch.cuda.synchronize()
    for i, r in enumerate(res):
        ref = cases[i % 2][1]
        assert int(r["status"].item()) == 0
        _assert_bit_exact({k: r[k].cpu().numpy() for k in ("loss", "grad")}, ref, ["loss", "grad"])
        assert r["loss_sum"].cpu().numpy().tobytes() == np.float32([wave_order_sum(ref["loss"])]).tobytes()


def test_v2_fwd_bwd_two_streams(gpu, oracle):
    B, T, D = 5, 150, 6
    table = np.array(dict(F4_TABLES)["long_durations"], np.int32)
    I = np.array([150, 149, 97, 70, 20], np.int32)
    rng = np.random.default_rng(3)
    O = np.array([int(table[rng.integers(0, D, size=i)].sum()) for i in I], np.int32)
    mt = int(O.max())
    xs = [_softmax_logits(np.random.default_rng(s), (B, T, D)) for s in (1, 2)]
    refs = [oracle.v2_fwd_bwd(x, table, I, O, mt, 0, True, False) for x in xs]
    assert not np.array_equal(refs[0]["loss"], refs[1]["loss"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    dx, tb, il, ol = [t(x) for x in xs], t(table), t(I), t(O)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    res = []
    for _ in range(2):
        for x, s in zip(dx, streams):
            with torch.cuda.stream(s):
                res.append(gpu.v2_fwd_bwd(x, tb, il, ol, 0, allow_skip=True, max_total=mt))
    torch.cuda.synchronize()
    for i, r in enumerate(res):
        assert int(r["status"].item()) == 0
        _same_v2({k: r[k].cpu().numpy() for k in ("loss", "grad")}, refs[i % 2], ["loss", "grad"])


# ---- the mirror's out= tensors: cells outside the extent hold their contract values ------------
def _nan_like(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(-1).view(I32).fill_(0x7FC00000)  # a NaN as f32; as i32 a value no output holds
    return t


def test_mirror_outputs_fwd_bwd(gpu, oracle):
    B, T, U = 4, 60, 65
    S, P = np.array([60, 41, 33, 7]), np.array([60, 40, 17, 1])
    lt = oracle.synth_log_trans(B, T, U, seed=65)
    lo = (np.random.default_rng(65).standard_normal((B, T, U)) * 15 - 40).astype(np.float32)
    out = {"loss": _nan_like((B,), F32), "grad": _nan_like((B, T, U, 2), F32),
           "grad_obs": _nan_like((B, T, U), F32), "log_alpha": _nan_like((B, T, U), F32),
           "log_beta": _nan_like((B, T, U), F32)}
    r = gpu.ssnt_fwd_bwd(_t(lt), _t(S, I32), _t(P, I32), _t(lo), debug=True, check=True, out=out)
    g = {k: r[k].cpu().numpy() for k in out}
    outside = np.zeros((B, T, U), bool)
    for b in range(B):
        outside[b, S[b]:], outside[b, :, P[b]:] = True, True
    assert not g["grad"][outside].any()
    assert not g["grad_obs"][outside].any()
    assert np.all(np.isneginf(g["log_alpha"][outside])) and np.all(np.isneginf(g["log_beta"][outside]))
    assert not np.isnan(g["grad"]).any() and not np.isnan(g["loss"]).any()
    _assert_bit_exact(g, oracle.fwd_bwd_xf(lt, S, P, log_obs=lo, debug=True), list(out))


def test_mirror_outputs_viterbi_and_sample(gpu):
    c = SC.reuse()
    lt, lo, S, P, K = c["lt"], c["lo"], c["S"], c["P"], c["K"]
    B, T, U, _ = lt.shape
    steps, places = np.arange(T)[None, :] >= S[:, None], np.arange(U)[None, :] >= P[:, None]
    out = {"log_prob": _nan_like((B,), F32), "position": _nan_like((B, T), I32), "duration": _nan_like((B, U), I32)}
    r = gpu.ssnt_viterbi_align(_t(lt), _t(S), _t(P), _t(lo), check=True, out=out)
    g = {k: r[k].cpu().numpy() for k in out}
    assert np.all(g["position"][steps] == -1) and np.all(g["duration"][places] == 0)
    _same_viterbi(g, VR.dp(lt, S, P, lo))
    out = {"log_prob": _nan_like((B, K), F32), "position": _nan_like((B, K, T), I32),
           "duration": _nan_like((B, K, U), I32)}
    r = gpu.ssnt_sample_align(_t(lt), _t(S), _t(P), K, _t(lo), uniform=_t(c["u"]), check=True, out=out)
    g = {k: r[k].cpu().numpy() for k in out}
    assert np.all(g["position"][np.broadcast_to(steps[:, None, :], (B, K, T))] == -1)
    assert np.all(g["duration"][np.broadcast_to(places[:, None, :], (B, K, U))] == 0)
    _check_sample(c, g, where="mirror out=")


def test_mirror_outputs_v2(gpu, oracle):
    logits, table, I, O, mt, allow_skip, test_mode = _v2_case("long_durations-band")
    B, T, D = logits.shape
    X = mt + 1
    steps = np.arange(T)[None, :] >= I[:, None]
    assert steps.any()
    args = (_t(logits), _t(table), _t(I), _t(O), 0)
    out = {"loss": _nan_like((B,), F32), "grad": _nan_like((B, T, D), F32),
           "log_alpha": _nan_like((B, T + 1, X), F32), "log_beta": _nan_like((B, T + 1, X), F32)}
    r = gpu.v2_fwd_bwd(*args, allow_skip=True, max_total=mt, debug=True, check=True, out=out)
    for k in out:
        assert r[k].data_ptr() == out[k].data_ptr()
    g = {k: r[k].cpu().numpy() for k in out}
    ref = oracle.v2_fwd_bwd(logits, table, I, O, mt, 0, True, False, debug=True)
    rows = np.arange(T + 1)[None, :] > I[:, None]  # (row r holds the totals after r steps)
    assert np.all(np.isneginf(ref["log_alpha"][rows])) and np.all(np.isneginf(ref["log_beta"][rows]))
    assert not g["grad"][steps].any() and not np.isnan(g["grad"]).any()
    assert np.all(np.isneginf(g["log_alpha"][rows])) and np.all(np.isneginf(g["log_beta"][rows]))
    _same_v2(g, ref, list(out))
    with pytest.raises(ValueError):
        gpu.v2_fwd_bwd(*args, max_total=mt, out={"grad": torch.empty((B, T, D + 1), device=DEV)})
    out = {"log_prob": _nan_like((B,), F32), "duration_class": _nan_like((B, T), I32),
           "duration": _nan_like((B, T), I32), "total": _nan_like((B,), I32)}
    r = gpu.v2_viterbi_align(*args, allow_skip=True, max_total=mt, check=True, out=out)
    g = {k: r[k].cpu().numpy() for k in out}
    assert np.all(g["duration_class"][steps] == -1) and np.all(g["duration"][steps] == 0)
    _same_v2_viterbi(g, V2R.dp(logits, table, I, O, mt, 0, True, False))
