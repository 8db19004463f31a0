"""The lattice kernels across the input value range (tests/value_cases.py), not one softmax.

Every other GPU parity test draws log_softmax of N(0, 1.5^2) logits: factors between e^-6 and 1.
Here the same bars hold on saturated softmaxes, positive scores, exponents of 1e4 .. 1e6 per step,
neighbouring terms 2^230 apart, the live / dead boundary of xf_exp and NaN in live cells:

  ssnt_fwd_bwd (streaming, two-wave and segmented kernel; `kernel_variant`) and v2_fwd_bwd
      BIT-EXACT against the split-exponent oracle on loss, grad, grad_obs, log_alpha, log_beta, status
      word 0; NaN / < -1e6 / > +1e6 inputs return the bits of the -inf / +1e6 inputs;
      ssnt_fwd_bwd_debug64_device within test_gpu_fwd_bwd.py's _check_debug64
  ssnt_viterbi_align, ssnt_nbest_align, v2_viterbi_align, v2_nbest_align
      bit-identical log-probabilities and identical paths against the f32 DPs of their own files

The shapes are the smallest that reach each code path of the streaming kernel (K = 1, 2, 4, the
narrow form, rows in LDS and in the workspace) and of the segmented kernel (one and two positions per
lane); within a batch S mod 4 takes every value the batch size allows, because the streaming chains
normalise every 4th step. tests/test_value_cases_ref.py holds the references to every condition
used here on the CPU. The sampler and expected-cost entries run the same classes in their own files."""
import functools

import numpy as np
import pytest

import nbest_ref as NR
import v2_nbest_ref as V2NR
import v2_viterbi_ref as V2VR
import value_cases as VC
import viterbi_ref as VR
from test_gpu_fwd_bwd import _assert_bit_exact, _check_debug64, _run_debug64, _run_gpu
from test_gpu_fwd_bwd import kernel_variant  # noqa: F401  (autouse: every case on every kernel)
from test_gpu_nbest_align import _run as _run_nbest
from test_gpu_nbest_align import _same as _same_nbest
from test_gpu_v2_fwd_bwd import _run as _run_v2
from test_gpu_v2_fwd_bwd import _same as _same_v2
from test_gpu_v2_nbest_align import _run as _run_v2_nbest
from test_gpu_v2_nbest_align import _same as _same_v2_nbest
from test_gpu_v2_viterbi import _run as _run_v2_viterbi
from test_gpu_v2_viterbi import _same as _same_v2_viterbi
from test_gpu_viterbi import _run as _run_viterbi
from test_gpu_viterbi import _same as _same_viterbi

pytestmark = pytest.mark.gpu

F_TERM = 1
KEYS = ["loss", "grad", "log_alpha", "log_beta"]

SHAPES = [            # (B, T, U)
    (4, 48, 64),      # streaming K=1, rows in LDS
    (4, 48, 80),      # streaming K=2 (the headline instance)
    (4, 48, 81),      # the narrow form (NV=1)
    (4, 48, 160),     # K=4, NC=2 / NH=2
    (3, 40, 256),     # K=4 upper edge; past the LDS boundary: rows in the workspace
    (2, 40, 300),     # segmented, one position per lane
    (2, 30, 700),     # segmented, two per lane (the two-wave kernel stops at U = 512)
]
WS_SHAPE = (3, 320, 80)  # workspace mode at the headline width
WS_CLASSES = ("peaked30", "patches", "alt_rows")
BOTH_FLAGS = ("peaked30", "patches", "threshold")  # the classes that also run without the terminal emit
META_SHAPES = [(4, 48, 80), (2, 40, 300)]
DEBUG64_SHAPES = [(3, 48, 80), (2, 40, 300)]
DEBUG64_CLASSES = ("peaked30", "plus88", "minus1e4", "alt_rows")


def _id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def _skip_unsupported(variant, shape):
    if variant == 1 and shape[2] > 512:
        pytest.skip("the two-wave kernel stops at U = 512")


# what the default dispatch must have run without log_obs (gpu.last_fwd_bwd_kernel()): the form
# each shape is there for
FORMS = {
    (4, 48, 64): ("k_fwd_bwd_stream<K=1,", "LDS=1", "NV=0"),
    (4, 48, 80): ("k_fwd_bwd_stream<K=2,", "LDS=1", "NV=0"),
    (4, 48, 81): ("k_fwd_bwd_stream<K=2,", "LDS=1", "NV=1"),
    (4, 48, 160): ("k_fwd_bwd_stream<K=4,", "LDS=1", "NC=2,NH=2"),
    (3, 40, 256): ("k_fwd_bwd_stream<K=4,", "LDS=0", "NC=2,NH=2"),
    WS_SHAPE: ("k_fwd_bwd_stream<K=2,", "LDS=0"),
    (2, 40, 300): ("k_fwd_bwd_wide<K=1,",),
    (2, 30, 700): ("k_fwd_bwd_wide<K=2,",),
    (2, 300, 8): ("k_fwd_bwd_stream<K=1,", "LDS=1"),
}


def _assert_streaming(gpu, variant, shape, obs=False):
    """The default dispatch runs the streaming kernel up to U = 256, in the form the shape is meant
    to reach: the case cannot pass on another kernel."""
    if variant != 0:
        return
    name = gpu.last_fwd_bwd_kernel()
    if shape[2] <= 256:
        assert name.startswith("k_fwd_bwd_stream<"), name
    if not obs:  # (with log_obs the rings differ, and with them the LDS boundary)
        assert all(part in name for part in FORMS[shape]), (name, FORMS[shape])


@functools.lru_cache(maxsize=8)
def _case(shape, trans, kind="ragged", obs=None, flags=F_TERM):
    """Inputs and the oracle's outputs (debug rows included), once for the three kernels."""
    import oracle as O
    B, T, U = shape
    lt = O.synth_log_trans(B, T, U, seed=T + U)
    if trans != "base":
        lt = VC.lattice(trans, lt)
    lo = None if obs is None else VC.obs(obs, (B, T, U))
    S, P = VC.lengths(B, T, U, kind)
    o = O.fwd_bwd_xf(lt, S, P, log_obs=lo, flags=flags, debug=True)
    return lt, lo, S, P, o


TRANSITION_CASES = ([(s, n) for s in SHAPES for n in VC.LATTICE_CLASSES] + [(WS_SHAPE, n) for n in WS_CLASSES])


@pytest.mark.parametrize("shape,name", TRANSITION_CASES, ids=_id)
def test_transition_classes_bit_exact(gpu, kernel_variant, shape, name):  # noqa: F811
    _skip_unsupported(kernel_variant, shape)
    for kind in VC.length_kinds(name):
        for flags in ((F_TERM, 0) if name in BOTH_FLAGS else (F_TERM,)):
            lt, _, S, P, o = _case(shape, name, kind, None, flags)
            g = _run_gpu(gpu, lt, S, P, flags=flags)
            _assert_streaming(gpu, kernel_variant, shape)
            _assert_bit_exact(g, o, KEYS)
            if flags == F_TERM:  # the product instance: no debug rows (other code in the segmented kernel)
                g = _run_gpu(gpu, lt, S, P, flags=flags, debug=False)
                _assert_streaming(gpu, kernel_variant, shape)
                _assert_bit_exact(g, o, ["loss", "grad"])


def test_near_envelope_bit_exact(gpu, kernel_variant):  # noqa: F811
    # cumulative log-probability -2.96e8, a live exponent of -4.3e8: the closest a test goes to
    # XF_EZERO = -2^29 from the inside (DESIGN.md 3 "Input domain")
    import oracle as O
    ne = VC.NEAR_ENVELOPE
    lt = VC.lattice("near_envelope", O.synth_log_trans(*ne["shape"], seed=1))
    o = O.fwd_bwd_xf(lt, ne["S"], ne["P"], debug=True)
    assert np.all(o["loss"] > 2.9e8) and np.all(np.isfinite(o["loss"]))
    g = _run_gpu(gpu, lt, ne["S"], ne["P"])
    _assert_streaming(gpu, kernel_variant, ne["shape"])
    _assert_bit_exact(g, o, KEYS)
    _assert_bit_exact(_run_gpu(gpu, lt, ne["S"], ne["P"], debug=False), o, ["loss", "grad"])


@pytest.mark.parametrize("trans", ["base", "peaked30"])
@pytest.mark.parametrize("obs", list(VC.OBS))
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_obs_classes_bit_exact(gpu, kernel_variant, shape, obs, trans):  # noqa: F811
    _skip_unsupported(kernel_variant, shape)
    lt, lo, S, P, o = _case(shape, trans, "ragged", obs)
    g = _run_gpu(gpu, lt, S, P, lo)
    _assert_streaming(gpu, kernel_variant, shape, obs=True)
    _assert_bit_exact(g, o, KEYS + ["grad_obs"])


@pytest.mark.parametrize("name", VC.CLEANED)
@pytest.mark.parametrize("shape", META_SHAPES, ids=_id)
def test_nan_and_out_of_range_inputs_read_as_neg_inf_and_the_clamp(gpu, kernel_variant, shape, name):  # noqa: F811
    # on the GPU outputs alone: NaN and values below -1e6 are -inf, values above +1e6 are +1e6
    is_obs = name in VC.OBS
    lt, lo, S, P, _ = _case(shape, "base" if is_obs else name, "ragged", name if is_obs else None)
    keys = KEYS + (["grad_obs"] if is_obs else [])
    for debug in (True, False):
        a = _run_gpu(gpu, lt, S, P, lo, debug=debug)
        b = _run_gpu(gpu, VC.cleaned(lt), S, P, VC.cleaned(lo), debug=debug)
        for k in (keys if debug else [k for k in keys if not k.startswith("log_")]):
            assert a[k].tobytes() == b[k].tobytes(), (k, debug)


@pytest.mark.parametrize("name", DEBUG64_CLASSES)
@pytest.mark.parametrize("shape", DEBUG64_SHAPES, ids=_id)
def test_debug64_value_classes(gpu, oracle, kernel_variant, shape, name):  # noqa: F811
    lt, _, S, P, _ = _case(shape, name)
    g = _run_debug64(gpu, lt, S, P)
    worst = _check_debug64(g, lt, S, P, oracle)
    print(shape, name, gpu.last_fwd_bwd_kernel(), worst)


# ---- the v2 duration-class lattice ----------------------------------------------------------------
V2_SHAPES = [(4, 40, 8, 4), (3, 24, 16, 7)]  # (B, I, D, planted duration per step)
V2_MODES = {"band": (False, True), "test_mode": (True, True), "no_skip": (False, False)}  # test_mode, allow_skip


@functools.lru_cache(maxsize=None)
def _v2_case(shape, name, mode):
    """Teacher-forced logits of ragged synth_durations lengths (utterance 0 full), one value class."""
    import oracle as O
    B, Imax, D, per_step = shape
    test_mode, allow_skip = V2_MODES[mode]
    d = O.synth_durations(B, Imax, per_step * Imax, D, seed=Imax)
    base = O.synth_v2_step_logits(d, D, seed=Imax + 1)
    logits = base if name == "base" else VC.v2(name, base)
    I = np.array([Imax, Imax - 5, Imax - 2, Imax - 11][:B], np.int32)
    Ol = np.array([int(d[b, :I[b]].sum()) for b in range(B)], np.int32)
    mt = int(Ol.max()) + (20 if test_mode else 3)
    return logits, np.arange(D, dtype=np.int32), I, Ol, mt, allow_skip, test_mode


class TestV2:
    @pytest.fixture(autouse=True)
    def kernel_variant(self):
        """The v2 entries and the path entries have one kernel each: no variants to force."""
        return 0

    @pytest.mark.parametrize("mode", list(V2_MODES))
    @pytest.mark.parametrize("name", list(VC.V2))
    @pytest.mark.parametrize("shape", V2_SHAPES, ids=_id)
    def test_v2_fwd_bwd_bit_exact(self, gpu, oracle, shape, name, mode):
        logits, table, I, Ol, mt, allow_skip, test_mode = _v2_case(shape, name, mode)
        o = oracle.v2_fwd_bwd(logits, table, I, Ol, mt, 0, allow_skip, test_mode, debug=True)
        g = _run_v2(gpu, logits, table, I, Ol, 0, allow_skip, test_mode, mt)
        _same_v2(g, o, KEYS)
        if name not in VC.CLEANED:
            assert np.all(np.isfinite(g["loss"]))
        else:  # on the GPU outputs alone: the bits of the -inf / +1e6 inputs
            c = _run_v2(gpu, VC.cleaned(logits), table, I, Ol, 0, allow_skip, test_mode, mt)
            for k in KEYS:
                assert g[k].tobytes() == c[k].tobytes(), k
        g = _run_v2(gpu, logits, table, I, Ol, 0, allow_skip, test_mode, mt, debug=False)
        _same_v2(g, o, ["loss", "grad"])

    # ---- the exact path entries: f32 DPs, finite or -inf inputs only ------------------------------
    @pytest.mark.parametrize("name", VC.PATH_CLASSES)
    @pytest.mark.parametrize("shape", META_SHAPES, ids=_id)
    def test_viterbi_and_nbest_value_classes(self, gpu, shape, name):
        # (`zeros`: every path ties, so the paths returned are the tie rule's)
        lt, _, S, P, _ = _case(shape, name)
        _same_viterbi(_run_viterbi(gpu, lt, S, P, check=True), VR.dp(lt, S, P), (shape, name))
        for N in (1, 4):
            _same_nbest(_run_nbest(gpu, lt, S, P, N, check=True), NR.dp(lt, S, P, N), (shape, name, N))

    @pytest.mark.parametrize("mode", ["band", "test_mode"])
    @pytest.mark.parametrize("name", VC.PATH_CLASSES)
    def test_v2_viterbi_and_nbest_value_classes(self, gpu, name, mode):
        logits, table, I, Ol, mt, allow_skip, test_mode = _v2_case(V2_SHAPES[0], name, mode)
        g = _run_v2_viterbi(gpu, logits, table, I, Ol, mt, 0, allow_skip, test_mode, check=True)
        _same_v2_viterbi(g, V2VR.dp(logits, table, I, Ol, mt, 0, allow_skip, test_mode), (name, mode))
        assert np.all(g["log_prob"] > -np.inf)
        for N in (1, 4):
            g = _run_v2_nbest(gpu, logits, table, I, Ol, mt, N, 0, allow_skip, test_mode, check=True)
            _same_v2_nbest(g, V2NR.dp(logits, table, I, Ol, mt, 0, allow_skip, test_mode, N), (name, mode, N))
