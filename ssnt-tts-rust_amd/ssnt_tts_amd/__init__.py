"""ssnt_tts_amd -- MI355X-native SSNT alignment engine, Python host mirror.

The function names, argument order and meaning mirror the reference's Python op wrappers
``ssnt_tts_tensorflow`` (ssnt-tts-tensorflow/ssnt_tts_tensorflow/__init__.py:8,24,33,76,85,99,
130), over torch device tensors instead of TF graph tensors. Every call goes through the C ABI
of ``lib/libssnt_tts_c.so`` (include/ssnt_tts_c.h) on torch's current HIP stream; there is no CPU
fallback. Added beside them: the lattice forward-backward (``ssnt_fwd_bwd``,
``SSNTLatticeLoss``), the same on a band of R columns per step in O(T*R) work and memory
(``ssnt_fwd_bwd_band``, ``SSNTBandLatticeLoss``, ``ssnt_band_lattice_loss``, with the pure-torch
helpers ``ssnt_band_from_positions``, ``ssnt_band_gather`` and ``ssnt_band_scatter``),
the exact best path over the same lattice (``ssnt_viterbi_align``) and inside a band of it
(``ssnt_viterbi_align_band``, with ``ssnt_band_edge_contact`` to tell a band that is too narrow),
the exact N best alignments (``ssnt_nbest_align``), alignments drawn from its posterior
(``ssnt_sample_align``), the posterior expectation of an additive path cost with its gradients
(``ssnt_expected_cost``, ``SSNTExpectedCost``, ``ssnt_alignment_entropy``), the posterior
distribution of every position's duration (``ssnt_duration_posterior``, with
``ssnt_duration_class_targets`` as the bridge to v2 classes), the counterparts of the first three on the v2
duration-class lattice (``v2_fwd_bwd``, ``v2_viterbi_align``, ``v2_sample_align``), the exact N
best duration paths on it (``v2_nbest_align``), the expected cost of a duration path on it
(``v2_expected_cost``, ``V2ExpectedCost``, ``v2_duration_entropy``) and a fused multi-step decode
(``lattice_beam_search_decode``).

Errors the reference raises by panicking (v2 "no candidate", upsample duration mismatch,
out-of-range branch) are raised here as ``SsntError`` when ``check=True`` (the default), which
synchronises the stream; pass ``check=False`` to stay asynchronous.
"""
from __future__ import annotations

import ctypes

import torch

from ._lib import SsntError, last_fwd_bwd_kernel, load, load_ab, status_string, use_ab  # noqa: F401

FLAG_TERMINAL_EMIT = 1
FLAG_ZERO_INFINITY = 2

__all__ = [
    "beam_search_decode", "extract_best_beam_branch", "ssnt_tts_v2_beam_search_decode",
    "order_beam_branch", "upsample_source_indexes", "tone_latent_beam_search_decode",
    "levenshtein_edit_distance", "ssnt_fwd_bwd", "ssnt_viterbi_align", "ssnt_sample_align",
    "ssnt_nbest_align", "SSNTLatticeLoss",
    "ssnt_fwd_bwd_band", "SSNTBandLatticeLoss", "ssnt_band_lattice_loss",
    "ssnt_band_from_positions", "ssnt_band_gather", "ssnt_band_scatter",
    "ssnt_viterbi_align_band", "ssnt_band_edge_contact",
    "ssnt_expected_cost", "SSNTExpectedCost", "ssnt_expected_cost_loss", "ssnt_alignment_entropy",
    "ssnt_lattice_loss", "ssnt_duration_posterior", "ssnt_duration_class_targets",
    "lattice_beam_search_decode", "v2_lattice_beam_search_decode",
    "tone_latent_lattice_beam_search_decode", "v2_fwd_bwd", "v2_viterbi_align", "v2_sample_align",
    "v2_nbest_align", "V2DurationLoss",
    "v2_duration_loss",
    "v2_expected_cost", "V2ExpectedCost", "v2_expected_cost_loss", "v2_duration_entropy",
    "SsntError", "FLAG_TERMINAL_EMIT", "FLAG_ZERO_INFINITY",
]


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _dev(t, dtype, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor")
    if not t.is_cuda:
        raise ValueError(f"{name}: must be a GPU tensor (libssnt_tts_c has no CPU fallback)")
    if t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous()


def _status(dev):
    return torch.zeros(1, dtype=torch.int32, device=dev)


def _finish(where, rc, status, check):
    if rc != 0:
        raise SsntError(where, rc)
    if check:
        bits = int(status.item())  # synchronises
        code = load().ssnt_status_from_bits(bits)
        if code != 0:
            raise SsntError(where, code)


# ----------------------------------------------------------------------------------------------
# Reference API mirror (ssnt_tts_tensorflow/__init__.py)
# ----------------------------------------------------------------------------------------------
def beam_search_decode(h, log_prob_history, is_finished, t, u, max_t, beam_width, *, check=True):
    """One v1 emit/shift beam-search step (ssnt_tts_tensorflow/__init__.py:8-21 ->
    src/lib.rs:121-230). h (W,2) as in the reference op, or batched (B,W,2). max_t: int or
    0-d tensor (one input length for the batch, src/lib.rs:99) or a (B,) tensor.
    Returns (prediction, log_prob, next_t, next_u, next_is_finished, beam_branch)."""
    lib = load(require_gpu=True)
    squeeze = h.dim() == 2
    h = _dev(h if not squeeze else h.unsqueeze(0), torch.float32, "h")
    dev = h.device
    B, W, C = h.shape
    if W != beam_width or C != 2:
        raise ValueError("h must be (W,2) / (B,W,2) with W == beam_width")
    hist = _dev(log_prob_history.reshape(B, W), torch.float32, "log_prob_history")
    fin = _dev(is_finished.reshape(B, W), torch.bool, "is_finished")
    tt = _dev(t.reshape(B, W), torch.int32, "t")
    uu = _dev(u.reshape(B, W), torch.int32, "u")
    if isinstance(max_t, torch.Tensor) and max_t.numel() == B and max_t.dim() == 1:
        il = _dev(max_t, torch.int32, "max_t")
    else:
        il = torch.full((B,), int(max_t), dtype=torch.int32, device=dev)
    outs = [torch.empty((B, W), dtype=dt, device=dev) for dt in
            (torch.int32, torch.float32, torch.int32, torch.int32, torch.bool, torch.int32)]
    st = _status(dev)
    rc = lib.ssnt_beam_search_decode_device(_p(h), _p(hist), _p(fin), _p(tt), _p(uu), _p(il), B,
                                            W, *[_p(o) for o in outs], _p(st), _stream(dev))
    _finish("beam_search_decode", rc, st, check)
    return tuple(o[0] for o in outs) if squeeze else tuple(outs)


def extract_best_beam_branch(best_final_branch, beam_branch, t_history, beam_width, *,
                             check=True):
    """Backtrace of the best final beam (ssnt_tts_tensorflow/__init__.py:24-30 ->
    src/util.rs:20-33). beam_branch, t_history (U,W) -> (U,), (U,); batched (B,U,W) with
    best_final_branch (B,) also accepted."""
    lib = load(require_gpu=True)
    squeeze = beam_branch.dim() == 2
    bb = _dev(beam_branch if not squeeze else beam_branch.unsqueeze(0), torch.int32, "beam_branch")
    dev = bb.device
    B, U, W = bb.shape
    if W != beam_width:
        raise ValueError("beam_branch last dim must equal beam_width")
    th = _dev(t_history.reshape(B, U, W), torch.int32, "t_history")
    fb = torch.as_tensor(best_final_branch, dtype=torch.int32, device=dev).reshape(B).contiguous()
    ob = torch.empty((B, U), dtype=torch.int32, device=dev)
    ot = torch.empty((B, U), dtype=torch.int32, device=dev)
    st = _status(dev)
    rc = lib.ssnt_extract_best_beam_branch_device(_p(fb), _p(bb), _p(th), B, W, U, _p(ob), _p(ot),
                                                  _p(st), _stream(dev))
    _finish("extract_best_beam_branch", rc, st, check)
    return (ob[0], ot[0]) if squeeze else (ob, ot)


def ssnt_tts_v2_beam_search_decode(h, log_prob_history, is_finished, total_duration,
                                   duration_table, t, u, input_length, output_length, beam_width,
                                   duration_class_size, zero_duration_id, allow_skip, test_mode,
                                   *, check=True):
    """One v2 duration-class step (ssnt_tts_tensorflow/__init__.py:33-73 -> src/v2.rs:221-339).
    h (B,W,D). Returns (prediction, log_prob, next_t, next_u, next_is_finished,
    next_total_duration, beam_branch), each (B,W)."""
    lib = load(require_gpu=True)
    h = _dev(h, torch.float32, "h")
    dev = h.device
    B, W, D = h.shape
    if W != beam_width or D != duration_class_size:
        raise ValueError("h must be (B, beam_width, duration_class_size)")
    il = _dev(input_length, torch.int32, "input_length").reshape(B)
    # the reference wrapper zeroes output_length in test mode (__init__.py:47)
    ol = torch.zeros_like(il) if test_mode else _dev(output_length, torch.int32,
                                                     "output_length").reshape(B)
    args = [_dev(x.reshape(B, W), dt, n) for x, dt, n in (
        (log_prob_history, torch.float32, "log_prob_history"), (is_finished, torch.bool, "is_finished"),
        (total_duration, torch.int32, "total_duration"))]
    table = _dev(duration_table, torch.int32, "duration_table").reshape(D)
    tt = _dev(t.reshape(B, W), torch.int32, "t")
    uu = _dev(u.reshape(B, W), torch.int32, "u")
    outs = [torch.empty((B, W), dtype=dt, device=dev) for dt in
            (torch.int32, torch.float32, torch.int32, torch.int32, torch.bool, torch.int32,
             torch.int32)]
    st = _status(dev)
    rc = lib.ssnt_v2_beam_search_decode_device(
        _p(h), _p(args[0]), _p(args[1]), _p(args[2]), _p(table), _p(tt), _p(uu), _p(il), _p(ol),
        B, W, D, int(zero_duration_id), bool(allow_skip), bool(test_mode),
        *[_p(o) for o in outs], _p(st), _stream(dev))
    _finish("ssnt_tts_v2_beam_search_decode", rc, st, check)
    return tuple(outs)


def order_beam_branch(final_branch, beam_branch, beam_width, *, check=True):
    """Backtrace of every final beam (ssnt_tts_tensorflow/__init__.py:76-82 ->
    src/v2_util.rs:6-36). final_branch (B,W), beam_branch (B,T,W) -> (B,W,T)."""
    lib = load(require_gpu=True)
    bb = _dev(beam_branch, torch.int32, "beam_branch")
    dev = bb.device
    B, T, W = bb.shape
    fb = _dev(final_branch, torch.int32, "final_branch").reshape(B, W)
    out = torch.empty((B, W, T), dtype=torch.int32, device=dev)
    st = _status(dev)
    rc = lib.ssnt_order_beam_branch_device(_p(fb), _p(bb), B, W, T, _p(out), _p(st), _stream(dev))
    _finish("order_beam_branch", rc, st, check)
    return out


def upsample_source_indexes(duration, output_length, out_of_range_source_index, beam_width, *,
                            check=True):
    """Durations -> frame-to-input index map (ssnt_tts_tensorflow/__init__.py:85-96 ->
    src/v2_util.rs:39-66). duration (B,W,T), output_length (B,W); the output is
    (B,W,max(output_length)) prefilled with out_of_range_source_index like the TF op
    (upsample_source_indexes_op.cc:75,90-92)."""
    lib = load(require_gpu=True)
    d = _dev(duration, torch.int32, "duration")
    dev = d.device
    B, W, T = d.shape
    ol = _dev(output_length, torch.int32, "output_length").reshape(B, W)
    max_u = int(ol.max().item()) if ol.numel() else 0
    out = torch.full((B, W, max_u), int(out_of_range_source_index), dtype=torch.int32, device=dev)
    if max_u == 0:
        return out
    st = _status(dev)
    rc = lib.ssnt_upsample_source_indexes_device(_p(d), _p(ol), B, W, T, max_u, _p(out), _p(st),
                                                 _stream(dev))
    _finish("upsample_source_indexes", rc, st, check)
    return out


def tone_latent_beam_search_decode(h, log_prob_history, is_finished, t, u, input_length,
                                   beam_width, tone_class_size, empty_tone_id, *, check=True):
    """One tone-latent step (ssnt_tts_tensorflow/__init__.py:99-127 ->
    src/tone_latent.rs:144-234). h (B,W,C). Returns 6 (B,W) tensors."""
    lib = load(require_gpu=True)
    h = _dev(h, torch.float32, "h")
    dev = h.device
    B, W, C = h.shape
    if W != beam_width or C != tone_class_size:
        raise ValueError("h must be (B, beam_width, tone_class_size)")
    hist = _dev(log_prob_history.reshape(B, W), torch.float32, "log_prob_history")
    fin = _dev(is_finished.reshape(B, W), torch.bool, "is_finished")
    tt = _dev(t.reshape(B, W), torch.int32, "t")
    uu = _dev(u.reshape(B, W), torch.int32, "u")
    il = _dev(input_length, torch.int32, "input_length").reshape(B)
    outs = [torch.empty((B, W), dtype=dt, device=dev) for dt in
            (torch.int32, torch.float32, torch.int32, torch.int32, torch.bool, torch.int32)]
    st = _status(dev)
    rc = lib.ssnt_tone_latent_beam_search_decode_device(
        _p(h), _p(hist), _p(fin), _p(tt), _p(uu), _p(il), B, W, C, int(empty_tone_id),
        *[_p(o) for o in outs], _p(st), _stream(dev))
    _finish("tone_latent_beam_search_decode", rc, st, check)
    return tuple(outs)


def levenshtein_edit_distance(a, b, a_lengths, b_lengths, *, check=True):
    """Batched Levenshtein distance (ssnt_tts_tensorflow/__init__.py:130-134 ->
    src/edit_distance.rs:6-60). a, b (B,L); lengths (B,) -> (B,)."""
    lib = load(require_gpu=True)
    a = _dev(a, torch.int32, "a")
    dev = a.device
    B, L = a.shape
    b = _dev(b, torch.int32, "b").reshape(B, L)
    al = _dev(a_lengths, torch.int32, "a_lengths").reshape(B)
    bl = _dev(b_lengths, torch.int32, "b_lengths").reshape(B)
    if check and B and (bool((al < 0).any()) or bool((al > L).any()) or bool((bl < 0).any())
                        or bool((bl > L).any())):
        raise ValueError("lengths must be within [0, max_length] (src/edit_distance.rs:17-18)")
    out = torch.empty((B,), dtype=torch.int32, device=dev)
    if B == 0:
        return out
    if L == 0:
        return out.zero_()
    rc = lib.ssnt_levenshtein_edit_distance_device(_p(a), _p(b), _p(al), _p(bl), B, L, _p(out),
                                                   _stream(dev))
    if rc != 0:
        raise SsntError("levenshtein_edit_distance", rc)
    return out


# ----------------------------------------------------------------------------------------------
# Lattice forward-backward (DESIGN.md "Lattice semantics")
# ----------------------------------------------------------------------------------------------
def _workspace(dev, nbytes):
    """Row workspace for one call, from torch's caching allocator on the current stream: reuse
    is free after the first call, and a buffer is never shared by launches on different streams
    (the allocator tracks the stream each block was allocated on)."""
    if nbytes == 0:
        return None
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


_sum_states = {}


def _sum_state(dev, B):
    """Zeroed in-launch loss-sum state (ssnt_fwd_bwd_sum_state_size), one per (device, stream)."""
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    nbytes = int(load().ssnt_fwd_bwd_sum_state_size(B))
    t = _sum_states.get(key)
    if t is None or t.numel() < nbytes:
        t = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        _sum_states[key] = t
    return t


def _shaped(t, dtype, name, shape):
    """_dev, in `shape`: a new view only where that is not the tensor's shape already."""
    t = _dev(t, dtype, name)
    return t if t.shape == shape else t.reshape(shape)


def _lattice_inputs(log_trans, step_len, pos_len, log_obs, terminal_emit, zero_infinity=False):
    """The checked device tensors (lt, sl, pl, lo) of a call on the emit/shift lattice and its
    flags word."""
    lt = _dev(log_trans, torch.float32, "log_trans")
    B, T, U, two = lt.shape
    if two != 2:
        raise ValueError("log_trans must be (B,T,U,2)")
    sl = _shaped(step_len, torch.int32, "step_len", (B,))
    pl = _shaped(pos_len, torch.int32, "pos_len", (B,))
    lo = None if log_obs is None else _shaped(log_obs, torch.float32, "log_obs", (B, T, U))
    flags = (FLAG_TERMINAL_EMIT if terminal_emit else 0) | (FLAG_ZERO_INFINITY if zero_infinity else 0)
    return lt, sl, pl, lo, flags


def _v2_inputs(logits, duration_table, input_length, output_length, max_total):
    """The checked device tensors (lg, table, il, ol) of a call on the v2 duration-class lattice
    and its max_total: the given one, else max(output_length), read back from the device."""
    lg = _dev(logits, torch.float32, "logits")
    B, _, D = lg.shape
    table = _shaped(duration_table, torch.int32, "duration_table", (D,))
    il = _shaped(input_length, torch.int32, "input_length", (B,))
    ol = _shaped(output_length, torch.int32, "output_length", (B,))
    if max_total is None:
        max_total = int(ol.max().item()) if B > 0 else 0
    return lg, table, il, ol, int(max_total)


def _uniform(uniform, dev, shape, dims, generator):
    """The randomness of a sampler: the caller's `uniform` (checked against `shape`, which reads
    `dims` in the error message), else drawn on the device."""
    if uniform is None:
        return torch.rand(shape, device=dev, dtype=torch.float32, generator=generator)
    un = _dev(uniform, torch.float32, "uniform")
    if tuple(un.shape) != shape:
        raise ValueError(f"uniform must be {dims} = {shape}")
    return un


def _a(t):
    """An optional tensor as a pointer argument of a lattice call: its plain address (ctypes
    converts it by the argtypes every symbol of _lib.SIGNATURES has), None as NULL."""
    return None if t is None else t.data_ptr()


class _Call:
    """One call of a lattice entry point: the steps all of them share (DESIGN.md "Host call
    protocol"). ``buf`` hands out the outputs and registers the wanted ones in ``res``, the dict
    the public function returns; ``workspace`` queries and allocates; ``run`` takes or makes the
    status word, calls the library and checks what it returned."""

    ws, wsb = None, 0  # (no workspace unless workspace() makes one)

    def __init__(self, where, dev, out, check):
        self.where, self.dev, self.out, self.check, self.res = where, dev, dict(out or {}), check, {}

    def buf(self, key, shape, dtype=torch.float32, want=True):
        """Output `key`: the caller's out[key] when given (checked), else a new tensor, kept as
        res[key]; returns its address. Not wanted: None (NULL to the library), absent from res."""
        if not want:
            return None
        t = self.out.get(key)
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=self.dev)
        elif tuple(t.shape) != tuple(shape) or t.dtype != dtype or not t.is_contiguous():
            raise ValueError(f"out[{key!r}] must be a contiguous {str(dtype)[6:]} tensor of shape {shape}")
        self.res[key] = t
        return t.data_ptr()

    def workspace(self, query, *shape):
        """The workspace `query(*shape)` asks for. A call that needs none (no path, no gradient)
        does not ask: the library then gets NULL and 0 bytes."""
        self.wsb = int(query(*shape))
        self.ws = _workspace(self.dev, self.wsb)

    def run(self, fn, *args, tail=()):
        """fn(*args, workspace, workspace_bytes, status, *tail, stream), args and tail as the
        library takes them (addresses, integers). The status word is out["status"], zeroed, else a
        new one. Returns ``res``."""
        st = self.out.get("status")
        if st is None:
            st = _status(self.dev)
        else:
            st.zero_()
        rc = fn(*args, _a(self.ws), self.wsb, st.data_ptr(), *tail, _stream(self.dev))
        if rc != 0 or self.check:
            _finish(self.where, rc, st, self.check)
        self.res["status"] = st
        return self.res


def ssnt_fwd_bwd(log_trans, step_len, pos_len, log_obs=None, *, terminal_emit=True,
                 zero_infinity=False, need_grad=True, debug=False, check=False, out=None,
                 loss_sum=False, debug64=False):
    """Forward-backward over the emit/shift lattice.

    log_trans (B,T,U,2) f32 [emit, shift] natural-log probabilities; step_len / pos_len (B,)
    lattice extents S_b <= T, P_b <= U; log_obs (B,T,U) optional. Returns a dict with
    ``loss`` (B,) = -ln Z, ``grad`` (B,T,U,2) = d loss / d log_trans (if need_grad),
    ``grad_obs`` (if log_obs given and need_grad), ``log_alpha`` / ``log_beta`` (if debug).
    ``out`` may pass preallocated tensors under the same keys (reused, for benchmarking).
    ``loss_sum=True`` adds ``loss_sum`` (1,) = sum_b loss[b], formed inside the same launch in a
    fixed order (ssnt_fwd_bwd_sum_device).
    ``debug64=True`` (ssnt_fwd_bwd_debug64_device) returns ``loss``, ``log_alpha`` and
    ``log_beta`` as float64, formed on the GPU from the kernel's split-exponent state (the
    north_star's 1e-5 bar on log-alpha / log-beta is below an f32 ulp at BASELINE magnitudes).
    """
    if debug64 and (out is not None or loss_sum or debug):
        # (the debug64 entry has its own float64 outputs and no fused loss sum: the C entry
        # rejects loss_sum with SSNT_ERR_INVALID_ARG, and out= / debug= would be ignored)
        raise ValueError("debug64=True cannot be combined with out=, loss_sum=True or debug=True")
    lib = load(require_gpu=True)
    lt, sl, pl, lo, flags = _lattice_inputs(log_trans, step_len, pos_len, log_obs, terminal_emit,
                                            zero_infinity)
    B, T, U, _ = lt.shape
    name = "ssnt_fwd_bwd_debug64" if debug64 else "ssnt_fwd_bwd"
    wide = torch.float64 if debug64 else torch.float32
    c = _Call(name, lt.device, out, check)
    loss = c.buf("loss", (B,), wide)
    grad = c.buf("grad", (B, T, U, 2), want=need_grad)
    gobs = c.buf("grad_obs", (B, T, U), want=need_grad and lo is not None)
    la = c.buf("log_alpha", (B, T, U), wide, want=debug or debug64)
    lb = c.buf("log_beta", (B, T, U), wide, want=debug or debug64)
    c.workspace(getattr(lib, name + "_workspace_size"), B, T, U)
    fn, tail = getattr(lib, name + "_device"), ()
    if loss_sum:
        fn = lib.ssnt_fwd_bwd_sum_device
        tail = (c.buf("loss_sum", (1,)), _sum_state(lt.device, B).data_ptr())
    return c.run(fn, lt.data_ptr(), _a(lo), sl.data_ptr(), pl.data_ptr(), B, T, U, flags,
                 loss, grad, gobs, la, lb, tail=tail)


def ssnt_viterbi_align(log_trans, step_len, pos_len, log_obs=None, *, terminal_emit=True,
                       need_path=True, check=False, out=None):
    """Exact best path (Viterbi) over the emit/shift lattice.

    Inputs as ``ssnt_fwd_bwd``. Returns a dict with ``log_prob`` (B,) f32, the log-probability
    of the most probable monotone alignment; ``position`` (B,T) i32, the input position of every
    step on it (-1 for steps >= S_b); ``duration`` (B,U) i32, the steps each position holds (0
    for positions >= P_b); ``status``. An infeasible utterance gets -inf, -1 and 0. A tie keeps
    the emit. ``need_path=False`` computes ``log_prob`` only. ``out`` may pass preallocated
    tensors under the same keys."""
    lib = load(require_gpu=True)
    lt, sl, pl, lo, flags = _lattice_inputs(log_trans, step_len, pos_len, log_obs, terminal_emit)
    B, T, U, _ = lt.shape
    c = _Call("ssnt_viterbi_align", lt.device, out, check)
    lp = c.buf("log_prob", (B,))
    pos = c.buf("position", (B, T), torch.int32, want=need_path)
    dur = c.buf("duration", (B, U), torch.int32, want=need_path)
    if need_path:
        c.workspace(lib.ssnt_viterbi_align_workspace_size, B, T, U)
    return c.run(lib.ssnt_viterbi_align_device, lt.data_ptr(), _a(lo), sl.data_ptr(),
                 pl.data_ptr(), B, T, U, flags, lp, pos, dur)


def ssnt_nbest_align(log_trans, step_len, pos_len, num_best, log_obs=None, *, terminal_emit=True,
                     need_path=True, check=False, out=None):
    """The exact N best alignments over the emit/shift lattice.

    Inputs as ``ssnt_fwd_bwd``; ``num_best`` N in [1, 8] (U <= 1024 / 512 / 256 for N <= 2 / 4 /
    8). Returns a dict with ``log_prob`` (B,N) f32, the log-probabilities of the N most probable
    monotone alignments, non-increasing; ``position`` (B,N,T) i32 and ``duration`` (B,N,U) i32 as
    ``ssnt_viterbi_align``, per rank; ``count`` (B,) i32, the number of present ranks; ``status``.
    The alignments of an utterance are pairwise distinct; rank 0 is ``ssnt_viterbi_align``'s. A
    rank beyond the number of alignments with positive probability is absent (-inf, -1 and 0);
    an infeasible utterance has every rank absent. ``need_path=False`` computes ``log_prob`` and
    ``count`` only. ``out`` may pass preallocated tensors under the same keys (not ``count``)."""
    lib = load(require_gpu=True)
    lt, sl, pl, lo, flags = _lattice_inputs(log_trans, step_len, pos_len, log_obs, terminal_emit)
    B, T, U, _ = lt.shape
    N = int(num_best)
    shape_n = max(N, 0)  # (an N the library refuses: the call below reports it)
    c = _Call("ssnt_nbest_align", lt.device, out, check)
    lp = c.buf("log_prob", (B, shape_n))
    pos = c.buf("position", (B, shape_n, T), torch.int32, want=need_path)
    dur = c.buf("duration", (B, shape_n, U), torch.int32, want=need_path)
    if need_path:
        c.workspace(lib.ssnt_nbest_align_workspace_size, B, T, U, N)
    c.run(lib.ssnt_nbest_align_device, lt.data_ptr(), _a(lo), sl.data_ptr(), pl.data_ptr(),
          B, T, U, N, flags, lp, pos, dur)
    c.res["count"] = (c.res["log_prob"] > float("-inf")).sum(dim=1).to(torch.int32)
    return c.res


def ssnt_sample_align(log_trans, step_len, pos_len, num_samples, log_obs=None, *, uniform=None,
                      generator=None, terminal_emit=True, need_path=True, out=None, check=True):
    """Alignments drawn from the posterior of the emit/shift lattice.

    Inputs as ``ssnt_fwd_bwd``; ``num_samples`` K in [1, 64] paths per utterance. ``uniform``
    (B,K,T) f32 is the randomness, one number per sample and step (clamped to [0, 1 - 2^-24], NaN
    counts as 0); without it ``torch.rand((B,K,T), generator=generator)`` is drawn on the device.
    The call is a pure function of its tensors. Returns a dict with ``log_prob`` (B,K) f32, the
    log-probability of each drawn path; ``position`` (B,K,T) i32 and ``duration`` (B,K,U) i32 as
    ``ssnt_viterbi_align``, per sample; ``uniform``, the numbers used; ``status``. An infeasible
    utterance gets -inf, -1 and 0 for every sample. ``need_path=False`` writes ``log_prob`` only.
    ``out`` may pass preallocated tensors under the same keys."""
    lib = load(require_gpu=True)
    lt, sl, pl, lo, flags = _lattice_inputs(log_trans, step_len, pos_len, log_obs, terminal_emit)
    B, T, U, _ = lt.shape
    K = int(num_samples)
    c = _Call("ssnt_sample_align", lt.device, out, check)
    un = c.res["uniform"] = _uniform(uniform, lt.device, (B, K, T), "(B,K,T)", generator)
    lp = c.buf("log_prob", (B, K))
    pos = c.buf("position", (B, K, T), torch.int32, want=need_path)
    dur = c.buf("duration", (B, K, U), torch.int32, want=need_path)
    c.workspace(lib.ssnt_sample_align_workspace_size, B, T, U, K)
    return c.run(lib.ssnt_sample_align_device, lt.data_ptr(), _a(lo), sl.data_ptr(),
                 pl.data_ptr(), un.data_ptr(), B, T, U, K, flags, lp, pos, dur)


class SSNTLatticeLoss(torch.autograd.Function):
    """Autograd wrapper: per-utterance loss (B,), gradients computed in the same kernel launch.
    The launch's status word (bad lengths, a bounded intra-kernel wait that expired) is checked
    in backward, where the step synchronises anyway (check=False skips it)."""

    @staticmethod
    def forward(ctx, log_trans, step_len, pos_len, log_obs=None, terminal_emit=True,
                zero_infinity=False, check=True):
        need = log_trans.requires_grad or (log_obs is not None and log_obs.requires_grad)
        r = ssnt_fwd_bwd(log_trans.detach(), step_len, pos_len,
                         None if log_obs is None else log_obs.detach(),
                         terminal_emit=terminal_emit, zero_infinity=zero_infinity, need_grad=need)
        ctx.save_for_backward(r.get("grad"), r.get("grad_obs"), r["status"])
        ctx.check = check
        return r["loss"]

    @staticmethod
    def backward(ctx, grad_loss):
        g, go, st = ctx.saved_tensors
        if ctx.check:
            _finish("ssnt_lattice_loss", 0, st, True)
        gl = grad_loss.to(torch.float32)
        gt = None if g is None else g * gl[:, None, None, None]
        gobs = None if go is None else go * gl[:, None, None]
        return gt, None, None, gobs, None, None, None


def ssnt_lattice_loss(log_trans, step_len, pos_len, log_obs=None, terminal_emit=True,
                      zero_infinity=False, check=True):
    return SSNTLatticeLoss.apply(log_trans, step_len, pos_len, log_obs, terminal_emit,
                                 zero_infinity, check)


# ----------------------------------------------------------------------------------------------
# Forward-backward on a band of the emit/shift lattice
# ----------------------------------------------------------------------------------------------
def _band_start(band_start, B, T):
    """band_start as a checked (B,T) integer tensor (int32 where it is not one already)."""
    if not isinstance(band_start, torch.Tensor):
        raise TypeError("band_start: expected a torch.Tensor")
    if band_start.dtype.is_floating_point or band_start.dtype.is_complex or band_start.dtype == torch.bool:
        raise TypeError(f"band_start must be an integer tensor, not {band_start.dtype}")
    if tuple(band_start.shape) != (B, T):
        raise ValueError(f"band_start must be (B,T) = {(B, T)}, not {tuple(band_start.shape)}")
    return band_start


def _band_index(band_start, width, U):
    """(idx (B,T,R) int64 clamped into [0, U), inside (B,T,R) bool) of a band's columns."""
    if int(width) < 1:
        raise ValueError("width must be at least 1")
    r = torch.arange(int(width), device=band_start.device, dtype=torch.int64)
    idx = band_start.to(torch.int64)[:, :, None] + r
    inside = (idx >= 0) & (idx < U)
    return idx.clamp(0, max(U - 1, 0)), inside


def ssnt_band_from_positions(position, step_len, pos_len, width):
    """The band of `width` columns centred on an alignment (pure torch, any device).

    position (B,T) integer, the input position of every step (``ssnt_viterbi_align``'s
    ``position``; entries at steps >= S_b are not read); step_len / pos_len (B,). Returns
    band_start (B,T) i32 with ``band_start[s] = clamp(position[s] - width//2, 0,
    max(P - width, 0))`` and the value of step S-1 repeated beyond it. For a monotone alignment
    (position[0] = 0, steps of 0 or 1, position[S-1] = P-1) the band is valid for
    ``ssnt_fwd_bwd_band`` and contains the alignment."""
    if not isinstance(position, torch.Tensor) or position.dim() != 2:
        raise ValueError("position must be a (B,T) tensor")
    if position.dtype.is_floating_point or position.dtype == torch.bool:
        raise TypeError(f"position must be an integer tensor, not {position.dtype}")
    if int(width) < 1:
        raise ValueError("width must be at least 1")
    B, T = position.shape
    dev = position.device
    S = torch.as_tensor(step_len, device=dev).reshape(B).to(torch.int64).clamp(0, T)
    P = torch.as_tensor(pos_len, device=dev).reshape(B).to(torch.int64)
    hi = (P - int(width)).clamp_min(0)[:, None]
    bs = torch.minimum((position.to(torch.int64) - int(width) // 2).clamp_min(0), hi)
    if T > 0:
        step = torch.minimum(torch.arange(T, device=dev)[None, :], (S - 1).clamp_min(0)[:, None])
        bs = bs.gather(1, step)
    return bs.to(torch.int32)


def ssnt_band_gather(dense, band_start, width, fill):
    """Cut a band out of a dense lattice tensor (pure torch, any device): dense (B,T,U,...) ->
    (B,T,width,...) with out[b,s,r] = dense[b,s,band_start[b,s]+r], and `fill` where that column
    lies outside [0, U)."""
    if not isinstance(dense, torch.Tensor) or dense.dim() < 3:
        raise ValueError("dense must be (B,T,U,...)")
    B, T, U = dense.shape[:3]
    bs = _band_start(band_start, B, T)
    idx, inside = _band_index(bs, width, U)
    tail = dense.shape[3:]
    shape = idx.shape + (1,) * len(tail)
    if U == 0:
        return torch.full(idx.shape + tail, fill, dtype=dense.dtype, device=dense.device)
    out = dense.gather(2, idx.reshape(shape).expand(idx.shape + tail))
    return torch.where(inside.reshape(shape), out, torch.full((), fill, dtype=dense.dtype, device=dense.device))


def ssnt_band_scatter(band, band_start, U, fill=0):
    """The inverse of ``ssnt_band_gather`` (pure torch, any device): band (B,T,R,...) ->
    (B,T,U,...) with out[b,s,band_start[b,s]+r] = band[b,s,r] and `fill` outside the band; band
    columns outside [0, U) are dropped."""
    if not isinstance(band, torch.Tensor) or band.dim() < 3:
        raise ValueError("band must be (B,T,R,...)")
    B, T, R = band.shape[:3]
    U = int(U)
    if U < 0:
        raise ValueError("U must not be negative")
    bs = _band_start(band_start, B, T)
    tail = band.shape[3:]
    out = torch.full((B, T, U + 1) + tail, fill, dtype=band.dtype, device=band.device)
    if R > 0:
        idx, inside = _band_index(bs, R, U)
        idx = torch.where(inside, idx, torch.full_like(idx, U))  # outside: the spare column
        shape = idx.shape + (1,) * len(tail)
        out.scatter_(2, idx.reshape(shape).expand(idx.shape + tail), band)
    return out[:, :, :U].contiguous()


def ssnt_fwd_bwd_band(log_trans_band, band_start, step_len, pos_len, log_obs_band=None, *,
                      terminal_emit=True, zero_infinity=False, need_grad=True, check=False,
                      out=None):
    """Forward-backward over a band of the emit/shift lattice: work and memory
    O(T*R), the dense (B,T,U,2) tensor is never formed.

    log_trans_band (B,T,R,2) f32 and log_obs_band (B,T,R) (optional) hold band cell (s,r) =
    lattice cell (s, band_start[b,s] + r); band_start (B,T) integer; step_len S_b <= T; pos_len
    P_b (there is no U). A valid band has band_start[b,0] = 0, steps of 0 or 1 up to S_b - 1, and
    band_start[b,S_b-1] <= P_b - 1 < band_start[b,S_b-1] + R (``ssnt_band_from_positions`` makes
    one from an alignment; ``ssnt_band_gather`` / ``ssnt_band_scatter`` move tensors between the
    two layouts). R in [1, 256]. Returns a dict with ``loss`` (B,) = -ln of the mass of the paths
    inside the band, ``grad`` (B,T,R,2) and ``grad_obs`` (B,T,R) (with need_grad; the latter if
    log_obs_band is given) and ``status``: the bits of ``ssnt_fwd_bwd`` on the dense lattice that
    is -inf outside the band. Edges that leave the band have gradient 0 and are never read. An
    invalid band makes its utterance infeasible (loss +inf, or 0 with zero_infinity; gradients 0)
    and raises ``SsntError`` (SSNT_ERR_BAD_BAND) with ``check=True``. ``need_grad=False`` needs no
    workspace and returns the same ``loss`` bits. ``out`` may pass preallocated tensors under the
    same keys."""
    lib = load(require_gpu=True)
    lt = _dev(log_trans_band, torch.float32, "log_trans_band")
    if lt.dim() != 4 or lt.shape[3] != 2:
        raise ValueError("log_trans_band must be (B,T,R,2)")
    B, T, R, _ = lt.shape
    bs = _dev(_band_start(band_start, B, T), torch.int32, "band_start")
    sl = _shaped(step_len, torch.int32, "step_len", (B,))
    pl = _shaped(pos_len, torch.int32, "pos_len", (B,))
    lo = None
    if log_obs_band is not None:
        lo = _dev(log_obs_band, torch.float32, "log_obs_band")
        if tuple(lo.shape) != (B, T, R):
            raise ValueError(f"log_obs_band must be (B,T,R) = {(B, T, R)}")
    flags = (FLAG_TERMINAL_EMIT if terminal_emit else 0) | (FLAG_ZERO_INFINITY if zero_infinity else 0)
    c = _Call("ssnt_fwd_bwd_band", lt.device, out, check)
    loss = c.buf("loss", (B,))
    grad = c.buf("grad", (B, T, R, 2), want=need_grad)
    gobs = c.buf("grad_obs", (B, T, R), want=need_grad and lo is not None)
    if need_grad:
        c.workspace(lib.ssnt_fwd_bwd_band_workspace_size, B, T, R)
    return c.run(lib.ssnt_fwd_bwd_band_device, lt.data_ptr(), _a(lo), bs.data_ptr(), sl.data_ptr(),
                 pl.data_ptr(), B, T, R, flags, loss, grad, gobs)


def ssnt_viterbi_align_band(log_trans_band, band_start, step_len, pos_len, log_obs_band=None, *,
                            terminal_emit=True, need_path=True, max_pos=None, check=False, out=None):
    """Exact best path (Viterbi) inside a band of the emit/shift lattice: work
    and memory O(T*R), the dense (B,T,U,2) tensor is never formed.

    Inputs as ``ssnt_fwd_bwd_band``. Returns a dict with ``log_prob`` (B,) f32, the
    log-probability of the most probable alignment whose every cell lies in the band;
    ``position`` (B,T) i32 (with need_path), its absolute position ``band_start + r`` at every
    step (-1 for steps >= S_b), which ``ssnt_band_from_positions`` turns into the next band;
    ``duration`` (B,max_pos) i32 (with need_path and ``max_pos`` given), the steps each position
    holds; ``status``: the bits of ``ssnt_viterbi_align`` on the dense lattice that is -inf
    outside the band. An infeasible utterance gets -inf, -1 and 0; so does an utterance with an
    invalid band (SSNT_ERR_BAD_BAND with ``check=True``) or with P_b > max_pos
    (SSNT_ERR_BAD_LENGTH). ``need_path=False`` needs no workspace and returns the same
    ``log_prob`` bits. ``ssnt_band_edge_contact`` tells whether the band was too narrow. ``out``
    may pass preallocated tensors under the same keys."""
    lib = load(require_gpu=True)
    lt = _dev(log_trans_band, torch.float32, "log_trans_band")
    if lt.dim() != 4 or lt.shape[3] != 2:
        raise ValueError("log_trans_band must be (B,T,R,2)")
    B, T, R, _ = lt.shape
    bs = _dev(_band_start(band_start, B, T), torch.int32, "band_start")
    sl = _shaped(step_len, torch.int32, "step_len", (B,))
    pl = _shaped(pos_len, torch.int32, "pos_len", (B,))
    lo = None
    if log_obs_band is not None:
        lo = _dev(log_obs_band, torch.float32, "log_obs_band")
        if tuple(lo.shape) != (B, T, R):
            raise ValueError(f"log_obs_band must be (B,T,R) = {(B, T, R)}")
    if max_pos is not None and int(max_pos) < 0:
        raise ValueError("max_pos must not be negative")
    U = 0 if max_pos is None else int(max_pos)
    c = _Call("ssnt_viterbi_align_band", lt.device, out, check)
    lp = c.buf("log_prob", (B,))
    pos = c.buf("position", (B, T), torch.int32, want=need_path)
    dur = c.buf("duration", (B, U), torch.int32, want=need_path and max_pos is not None)
    if need_path:
        c.workspace(lib.ssnt_viterbi_align_band_workspace_size, B, T, R)
    return c.run(lib.ssnt_viterbi_align_band_device, lt.data_ptr(), _a(lo), bs.data_ptr(),
                 sl.data_ptr(), pl.data_ptr(), B, T, R, U, FLAG_TERMINAL_EMIT if terminal_emit else 0,
                 lp, pos, dur)


def ssnt_band_edge_contact(position, band_start, step_len, pos_len, width):
    """How often a path touches an edge of its band that has lattice beyond it (pure torch, any
    device): the sign that the band is too narrow.

    position (B,T) integer, absolute positions (``ssnt_viterbi_align_band``'s ``position``; -1
    marks an infeasible utterance); band_start (B,T) integer; step_len / pos_len (B,); ``width``
    = R. Returns (B,) i32: the number of steps s < S_b at which the path sits on column r = 0 with
    ``band_start[s] > 0``, or on column r = R-1 with ``band_start[s] + R < P_b``. 0 for an
    infeasible utterance."""
    if not isinstance(position, torch.Tensor) or position.dim() != 2:
        raise ValueError("position must be a (B,T) tensor")
    if position.dtype.is_floating_point or position.dtype == torch.bool:
        raise TypeError(f"position must be an integer tensor, not {position.dtype}")
    if int(width) < 1:
        raise ValueError("width must be at least 1")
    B, T = position.shape
    dev = position.device
    bs = _band_start(band_start, B, T).to(device=dev, dtype=torch.int64)
    S = torch.as_tensor(step_len, device=dev).reshape(B).to(torch.int64).clamp(0, T)
    P = torch.as_tensor(pos_len, device=dev).reshape(B).to(torch.int64)
    pos = position.to(torch.int64)
    live = (torch.arange(T, device=dev)[None, :] < S[:, None]) & (pos >= 0)
    r = pos - bs
    low = (r == 0) & (bs > 0)
    high = (r == int(width) - 1) & (bs + int(width) < P[:, None])
    return ((low | high) & live).sum(dim=1).to(torch.int32)


class SSNTBandLatticeLoss(torch.autograd.Function):
    """Autograd wrapper of ``ssnt_fwd_bwd_band``: per-utterance loss (B,), gradients in the band
    layout, computed in the same kernel launch. The status word (bad lengths, an invalid band) is
    checked in backward, where the step synchronises anyway (check=False skips it)."""

    @staticmethod
    def forward(ctx, log_trans_band, band_start, step_len, pos_len, log_obs_band=None,
                terminal_emit=True, zero_infinity=False, check=True):
        need = log_trans_band.requires_grad or (log_obs_band is not None and log_obs_band.requires_grad)
        r = ssnt_fwd_bwd_band(log_trans_band.detach(), band_start, step_len, pos_len,
                              None if log_obs_band is None else log_obs_band.detach(),
                              terminal_emit=terminal_emit, zero_infinity=zero_infinity, need_grad=need)
        ctx.save_for_backward(r.get("grad"), r.get("grad_obs"), r["status"])
        ctx.check = check
        return r["loss"]

    @staticmethod
    def backward(ctx, grad_loss):
        g, go, st = ctx.saved_tensors
        if ctx.check:
            _finish("ssnt_band_lattice_loss", 0, st, True)
        gl = grad_loss.to(torch.float32)
        gt = None if g is None else g * gl[:, None, None, None]
        gobs = None if go is None else go * gl[:, None, None]
        return gt, None, None, None, gobs, None, None, None


def ssnt_band_lattice_loss(log_trans_band, band_start, step_len, pos_len, log_obs_band=None,
                           terminal_emit=True, zero_infinity=False, check=True):
    return SSNTBandLatticeLoss.apply(log_trans_band, band_start, step_len, pos_len, log_obs_band,
                                     terminal_emit, zero_infinity, check)


def ssnt_expected_cost(log_trans, cost, step_len, pos_len, log_obs=None, *, terminal_emit=True,
                       need_grad=True, check=False, out=None):
    """The posterior expectation of an additive path cost on the emit/shift lattice, and its
    gradients (the expectation semiring).

    Inputs as ``ssnt_fwd_bwd``; ``cost`` (B,T,U,2) f32 is added to a path's cost when it takes the
    edge [b,s,p,k] (the terminal emit's cost counts iff ``terminal_emit``). Returns a dict with
    ``risk`` (B,) = E[cost of the path], ``loss`` (B,) = -ln Z, ``status`` and, with ``need_grad``,
    ``grad_trans`` (B,T,U,2) = d risk / d log_trans, ``grad_cost`` (B,T,U,2) = d risk / d cost (the
    edge posterior) and ``grad_obs`` (B,T,U) = d risk / d log_obs (if ``log_obs`` is given). An
    infeasible utterance gets risk 0, loss +inf and gradients 0. ``need_grad=False`` runs the
    forward sweep alone and returns the same bits of ``risk`` and ``loss``. ``out`` may pass
    preallocated tensors under the same keys."""
    lib = load(require_gpu=True)
    lt, sl, pl, lo, flags = _lattice_inputs(log_trans, step_len, pos_len, log_obs, terminal_emit)
    B, T, U, _ = lt.shape
    cs = _dev(cost, torch.float32, "cost")
    if tuple(cs.shape) != (B, T, U, 2):
        raise ValueError(f"cost must be (B,T,U,2) = {(B, T, U, 2)}")
    c = _Call("ssnt_expected_cost", lt.device, out, check)
    risk = c.buf("risk", (B,))
    loss = c.buf("loss", (B,))
    gt = c.buf("grad_trans", (B, T, U, 2), want=need_grad)
    gc = c.buf("grad_cost", (B, T, U, 2), want=need_grad)
    go = c.buf("grad_obs", (B, T, U), want=need_grad and lo is not None)
    if need_grad:
        c.workspace(lib.ssnt_expected_cost_workspace_size, B, T, U)
    return c.run(lib.ssnt_expected_cost_device, lt.data_ptr(), _a(lo), cs.data_ptr(),
                 sl.data_ptr(), pl.data_ptr(), B, T, U, flags, risk, loss, gt, gc, go)


def ssnt_duration_posterior(log_trans, step_len, pos_len, num_bins, log_obs=None, *,
                            terminal_emit=True, out=None, check=True):
    """The posterior distribution of every position's duration on the emit/shift lattice
    (DESIGN.md 2.10).

    Inputs as ``ssnt_fwd_bwd``; ``num_bins`` = D in [2, 256]. Returns a dict with ``dur_post``
    (B,U,D) f32, whose bin index is the duration: ``dur_post[b,p,d]`` = P(position p lasts exactly d
    steps) for d < D-1 (bin 0 is an exact 0) and ``dur_post[b,p,D-1]`` = P(it lasts at least D-1
    steps); ``loss`` (B,) = -ln Z with the bits of ``ssnt_expected_cost``'s; and ``status``. A row
    p < P_b sums to 1, rows p >= P_b are 0, and an infeasible utterance gets ``dur_post`` 0 and loss
    +inf. ``out`` may pass preallocated tensors under the same keys."""
    lib = load(require_gpu=True)
    lt, sl, pl, lo, flags = _lattice_inputs(log_trans, step_len, pos_len, log_obs, terminal_emit)
    B, T, U, _ = lt.shape
    D = int(num_bins)
    if not 2 <= D <= 256:
        raise ValueError("num_bins must be in [2, 256]")
    c = _Call("ssnt_duration_posterior", lt.device, out, check)
    dp = c.buf("dur_post", (B, U, D))
    loss = c.buf("loss", (B,))
    c.workspace(lib.ssnt_duration_posterior_workspace_size, B, T, U, D)
    return c.run(lib.ssnt_duration_posterior_device, lt.data_ptr(), _a(lo), sl.data_ptr(),
                 pl.data_ptr(), B, T, U, D, flags, dp, loss)


def ssnt_duration_class_targets(dur_post, duration_table):
    """Soft targets over a v2 ``duration_table`` from ``dur_post`` (B,U,D) of
    ``ssnt_duration_posterior``: pure torch, on any device. Returns ``(targets (B,U,C),
    residual (B,U))``: ``targets[..., i] = dur_post[..., duration_table[i]]`` for a table value
    below D-1, and 0 for a value >= D-1 (the tail bin is no exact duration); ``residual`` = the row
    sum of ``dur_post`` minus the row sum of ``targets``, the posterior mass no class represents.
    A table value that occurs twice raises ``ValueError`` (its mass would count twice)."""
    if not isinstance(dur_post, torch.Tensor) or dur_post.dim() != 3:
        raise ValueError("dur_post must be a (B,U,D) tensor")
    table = torch.as_tensor(duration_table, dtype=torch.int64).reshape(-1).cpu()
    if table.numel() and int(table.min()) < 0:
        raise ValueError("duration_table must be >= 0")
    if torch.unique(table).numel() != table.numel():
        raise ValueError("duration_table holds a value twice")
    D = dur_post.shape[-1]
    exact = (table < D - 1).to(dur_post.device)
    index = table.clamp(max=D - 1).to(dur_post.device)
    targets = dur_post.index_select(-1, index) * exact.to(dur_post.dtype)
    return targets, dur_post.sum(-1) - targets.sum(-1)


class SSNTExpectedCost(torch.autograd.Function):
    """Autograd wrapper: per-utterance risk (B,), differentiable with respect to log_trans, cost
    and log_obs; the gradients come from the same call. The status word is checked in backward,
    as SSNTLatticeLoss does (check=False skips it)."""

    @staticmethod
    def forward(ctx, log_trans, cost, step_len, pos_len, log_obs=None, terminal_emit=True, check=True):
        need = (log_trans.requires_grad or cost.requires_grad
                or (log_obs is not None and log_obs.requires_grad))
        r = ssnt_expected_cost(log_trans.detach(), cost.detach(), step_len, pos_len,
                               None if log_obs is None else log_obs.detach(),
                               terminal_emit=terminal_emit, need_grad=need)
        ctx.save_for_backward(r.get("grad_trans"), r.get("grad_cost"), r.get("grad_obs"), r["status"])
        ctx.check = check
        return r["risk"]

    @staticmethod
    def backward(ctx, grad_risk):
        gt, gc, go, st = ctx.saved_tensors
        if ctx.check:
            _finish("ssnt_expected_cost_loss", 0, st, True)
        gr = grad_risk.to(torch.float32)
        need_t, need_c, _, _, need_o = ctx.needs_input_grad[:5]
        dt = gt * gr[:, None, None, None] if need_t and gt is not None else None
        dc = gc * gr[:, None, None, None] if need_c and gc is not None else None
        do = go * gr[:, None, None] if need_o and go is not None else None
        return dt, dc, None, None, do, None, None


def ssnt_expected_cost_loss(log_trans, cost, step_len, pos_len, log_obs=None, terminal_emit=True,
                            check=True):
    """risk (B,) of ``ssnt_expected_cost``, differentiable (minimum-risk training, expected
    durations and positions)."""
    return SSNTExpectedCost.apply(log_trans, cost, step_len, pos_len, log_obs, terminal_emit, check)


def ssnt_alignment_entropy(log_trans, step_len, pos_len, log_obs=None, terminal_emit=True):
    """The entropy H (B,) of the alignment posterior, differentiable: H = ln Z - E[ln w(path)],
    with ln Z = -loss of ``ssnt_lattice_loss`` and E[ln w] = risk of ``ssnt_expected_cost_loss``
    for cost = log_trans, plus the log_obs of the entered cell on both edges that enter it (the
    terminal emit enters none). log_obs[b,0,0] belongs to every path and to no edge; it is in
    ln Z, so it is subtracted once."""
    cost = log_trans.to(torch.float32)
    first = None
    if log_obs is not None:
        B, T, U, _ = log_trans.shape
        lo = log_obs.to(torch.float32).reshape(B, T, U)
        first = lo[:, 0, 0]
        pad_s = torch.zeros_like(lo[:, :1])
        same = torch.cat([lo[:, 1:], pad_s], dim=1)                           # obs[s+1, p]
        nxt = torch.cat([same[:, :, 1:], torch.zeros_like(same[:, :, :1])], dim=2)  # obs[s+1, p+1]
        sl = step_len.to(device=lo.device, dtype=torch.int64).reshape(B)
        inner = torch.arange(T, device=lo.device)[None, :, None, None] < (sl[:, None, None, None] - 1)
        cost = cost + torch.where(inner, torch.stack([same, nxt], dim=-1), torch.zeros((), device=lo.device))
    loss = ssnt_lattice_loss(log_trans, step_len, pos_len, log_obs, terminal_emit)
    risk = ssnt_expected_cost_loss(log_trans, cost, step_len, pos_len, log_obs, terminal_emit)
    h = -loss - risk
    return h if first is None else h - first


# ----------------------------------------------------------------------------------------------
# F4: v2 duration-class forward-backward (DESIGN.md "Duration lattice")
# ----------------------------------------------------------------------------------------------
def v2_fwd_bwd(logits, duration_table, input_length, output_length, zero_duration_id, *,
               allow_skip=False, test_mode=False, max_total=None, zero_infinity=False,
               need_grad=True, debug=False, check=False, out=None):
    """Forward-backward over the v2 duration-class lattice: the sum over every class sequence the
    v2 decode could keep (src/v2.rs:94-166 move rules) of its probability.

    logits (B,T,D) per-step class log-probs (teacher-forced); duration_table (D,) >= 0;
    input_length / output_length (B,). ``max_total`` bounds the state totals (default
    max(output_length), read back from the device). Returns ``loss`` (B,) = -ln Z, ``grad``
    (B,T,D) = d loss / d logits (= minus the class posteriors), and with ``debug`` the rows
    ``log_alpha`` / ``log_beta`` (B,T+1,max_total+1). Rows of ``grad`` at steps >= I_b are 0.
    ``out`` may pass preallocated tensors under the same keys."""
    lib = load(require_gpu=True)
    lg, table, il, ol, mt = _v2_inputs(logits, duration_table, input_length, output_length, max_total)
    B, T, D = lg.shape
    c = _Call("v2_fwd_bwd", lg.device, out, check)
    loss = c.buf("loss", (B,))
    grad = c.buf("grad", (B, T, D), want=need_grad)
    la = c.buf("log_alpha", (B, T + 1, mt + 1), want=debug)
    lb = c.buf("log_beta", (B, T + 1, mt + 1), want=debug)
    c.workspace(lib.ssnt_v2_fwd_bwd_workspace_size, B, T, mt, bool(test_mode))
    return c.run(lib.ssnt_v2_fwd_bwd_device, lg.data_ptr(), table.data_ptr(), il.data_ptr(),
                 ol.data_ptr(), B, T, D, mt, int(zero_duration_id), bool(allow_skip), bool(test_mode),
                 FLAG_ZERO_INFINITY if zero_infinity else 0, loss, grad, la, lb)


def v2_viterbi_align(logits, duration_table, input_length, output_length, zero_duration_id, *,
                     allow_skip=False, test_mode=False, max_total=None, need_path=True,
                     check=False, out=None):
    """Exact best duration path (Viterbi) on the v2 duration-class lattice.

    Inputs as ``v2_fwd_bwd`` (``max_total`` defaults to max(output_length), read back from the
    device). Returns a dict with ``log_prob`` (B,) f32, the log-probability of the most probable
    class sequence the v2 move rules admit; ``duration_class`` (B,T) i32, its class at every step
    (-1 for steps >= I_b); ``duration`` (B,T) i32 = duration_table[class] (0 for steps >= I_b);
    ``total`` (B,) i32, its final total (= O_b in band mode); ``status``. An utterance without an
    admissible path gets -inf, -1, 0 and -1. A tie keeps the lower class (and the lower final
    total). ``need_path=False`` computes ``log_prob`` only. ``out`` may pass preallocated
    tensors under the same keys."""
    lib = load(require_gpu=True)
    lg, table, il, ol, mt = _v2_inputs(logits, duration_table, input_length, output_length, max_total)
    B, T, D = lg.shape
    c = _Call("v2_viterbi_align", lg.device, out, check)
    lp = c.buf("log_prob", (B,))
    cls = c.buf("duration_class", (B, T), torch.int32, want=need_path)
    dur = c.buf("duration", (B, T), torch.int32, want=need_path)
    tot = c.buf("total", (B,), torch.int32, want=need_path)
    if need_path:
        c.workspace(lib.ssnt_v2_viterbi_align_workspace_size, B, T, mt, bool(test_mode))
    return c.run(lib.ssnt_v2_viterbi_align_device, lg.data_ptr(), table.data_ptr(), il.data_ptr(),
                 ol.data_ptr(), B, T, D, mt, int(zero_duration_id), bool(allow_skip), bool(test_mode),
                 lp, cls, dur, tot)


def v2_nbest_align(logits, duration_table, input_length, output_length, zero_duration_id, num_best,
                   *, allow_skip=False, test_mode=False, max_total=None, need_path=True,
                   check=False, out=None):
    """The exact N best duration paths on the v2 duration-class lattice.

    Inputs as ``v2_viterbi_align``; ``num_best`` N in [1, 8]. Returns a dict with ``log_prob``
    (B,N) f32, the log-probabilities of the N most probable class sequences the v2 move rules
    admit, non-increasing; ``duration_class`` (B,N,T) i32, ``duration`` (B,N,T) i32 and ``total``
    (B,N) i32 as ``v2_viterbi_align``, per rank; ``count`` (B,) i32, the number of present ranks;
    ``status``. The class sequences of an utterance are pairwise distinct; rank 0 is
    ``v2_viterbi_align``'s. A rank beyond the number of admissible sequences with positive
    probability is absent (-inf, -1, 0 and -1); an utterance without an admissible path has every
    rank absent. ``need_path=False`` computes ``log_prob`` and ``count`` only. ``out`` may pass
    preallocated tensors under the same keys (not ``count``)."""
    lib = load(require_gpu=True)
    lg, table, il, ol, mt = _v2_inputs(logits, duration_table, input_length, output_length, max_total)
    B, T, D = lg.shape
    N = int(num_best)
    shape_n = max(N, 0)  # (an N the library refuses: the call below reports it)
    c = _Call("v2_nbest_align", lg.device, out, check)
    lp = c.buf("log_prob", (B, shape_n))
    cls = c.buf("duration_class", (B, shape_n, T), torch.int32, want=need_path)
    dur = c.buf("duration", (B, shape_n, T), torch.int32, want=need_path)
    tot = c.buf("total", (B, shape_n), torch.int32, want=need_path)
    if need_path:
        c.workspace(lib.ssnt_v2_nbest_align_workspace_size, B, T, mt, bool(test_mode), N)
    c.run(lib.ssnt_v2_nbest_align_device, lg.data_ptr(), table.data_ptr(), il.data_ptr(),
          ol.data_ptr(), B, T, D, mt, int(zero_duration_id), bool(allow_skip), bool(test_mode), N,
          lp, cls, dur, tot)
    c.res["count"] = (c.res["log_prob"] > float("-inf")).sum(dim=1).to(torch.int32)
    return c.res


def v2_sample_align(logits, duration_table, input_length, output_length, zero_duration_id,
                    num_samples, *, uniform=None, generator=None, allow_skip=False,
                    test_mode=False, max_total=None, need_path=True, check=False, out=None):
    """Duration paths drawn from the posterior of the v2 duration-class lattice.

    Inputs as ``v2_fwd_bwd`` (``max_total`` defaults to max(output_length), read back from the
    device); ``num_samples`` K in [1, 64] class sequences per utterance. ``uniform`` (B,K,T+1) f32
    is the randomness: [b,k,t] chooses the class of step t, [b,k,T] the final total (clamped to
    [0, 1 - 2^-24], NaN counts as 0); without it ``torch.rand((B,K,T+1), generator=generator)`` is
    drawn on the device. The call is a pure function of its tensors. Returns a dict with
    ``log_prob`` (B,K) f32, the log-probability of each drawn sequence; ``duration_class`` (B,K,T)
    i32 (-1 for steps >= I_b), ``duration`` (B,K,T) i32 = duration_table[class] (0 for steps >=
    I_b) and ``total`` (B,K) i32 as ``v2_viterbi_align``, per sample; ``uniform``, the numbers
    used; ``status``. An utterance without an admissible path gets -inf, -1, 0 and -1 for every
    sample. ``need_path=False`` writes ``log_prob`` only. ``out`` may pass preallocated tensors
    under the same keys."""
    lib = load(require_gpu=True)
    lg, table, il, ol, mt = _v2_inputs(logits, duration_table, input_length, output_length, max_total)
    B, T, D = lg.shape
    K = int(num_samples)
    c = _Call("v2_sample_align", lg.device, out, check)
    un = c.res["uniform"] = _uniform(uniform, lg.device, (B, K, T + 1), "(B,K,T+1)", generator)
    lp = c.buf("log_prob", (B, K))
    cls = c.buf("duration_class", (B, K, T), torch.int32, want=need_path)
    dur = c.buf("duration", (B, K, T), torch.int32, want=need_path)
    tot = c.buf("total", (B, K), torch.int32, want=need_path)
    c.workspace(lib.ssnt_v2_sample_align_workspace_size, B, T, mt, bool(test_mode), K)
    return c.run(lib.ssnt_v2_sample_align_device, lg.data_ptr(), table.data_ptr(), il.data_ptr(),
                 ol.data_ptr(), un.data_ptr(), B, T, D, mt, int(zero_duration_id), bool(allow_skip),
                 bool(test_mode), K, lp, cls, dur, tot)


class V2DurationLoss(torch.autograd.Function):
    """Autograd wrapper of v2_fwd_bwd: per-utterance loss (B,), gradients from the same launch."""

    @staticmethod
    def forward(ctx, logits, duration_table, input_length, output_length, zero_duration_id,
                allow_skip=False, test_mode=False, max_total=None, zero_infinity=False, check=True):
        r = v2_fwd_bwd(logits.detach(), duration_table, input_length, output_length,
                       zero_duration_id, allow_skip=allow_skip, test_mode=test_mode,
                       max_total=max_total, zero_infinity=zero_infinity,
                       need_grad=logits.requires_grad)
        ctx.save_for_backward(r.get("grad"), r["status"])
        ctx.check = check
        return r["loss"]

    @staticmethod
    def backward(ctx, grad_loss):
        g, st = ctx.saved_tensors
        if ctx.check:
            _finish("v2_duration_loss", 0, st, True)
        gl = None if g is None else g * grad_loss.to(torch.float32)[:, None, None]
        return gl, None, None, None, None, None, None, None, None, None


def v2_duration_loss(logits, duration_table, input_length, output_length, zero_duration_id,
                     allow_skip=False, test_mode=False, max_total=None, zero_infinity=False,
                     check=True):
    return V2DurationLoss.apply(logits, duration_table, input_length, output_length,
                                zero_duration_id, allow_skip, test_mode, max_total, zero_infinity,
                                check)


def v2_expected_cost(logits, cost, duration_table, input_length, output_length, zero_duration_id,
                     *, allow_skip=False, test_mode=False, max_total=None, need_grad=True,
                     check=False, out=None):
    """The posterior expectation of an additive per-step, per-class cost on the v2 duration-class
    lattice, and its gradients (the expectation semiring).

    Inputs as ``v2_fwd_bwd`` (``max_total`` defaults to max(output_length), read back from the
    device); ``cost`` (B,T,D) f32 is added to a path's cost when step t takes class i. Returns a
    dict with ``risk`` (B,) = E[cost of the path], ``loss`` (B,) = -ln Z (the bits of
    ``v2_fwd_bwd``), ``status`` and, with ``need_grad``, ``grad_logits`` (B,T,D) = d risk / d logits
    and ``grad_cost`` (B,T,D) = d risk / d cost (the class posterior). An utterance without an
    admissible path gets risk 0, loss +inf and gradients 0. A class of weight zero contributes an
    exact 0 whatever its cost holds. ``need_grad=False`` runs the forward sweep alone and returns
    the same bits of ``risk`` and ``loss``. ``out`` may pass preallocated tensors under the same
    keys."""
    lib = load(require_gpu=True)
    lg = _dev(logits, torch.float32, "logits")
    B, T, D = lg.shape
    cs = _dev(cost, torch.float32, "cost")
    if tuple(cs.shape) != (B, T, D):
        raise ValueError(f"cost must be (B,T,D) = {(B, T, D)}")
    lg, table, il, ol, mt = _v2_inputs(lg, duration_table, input_length, output_length, max_total)
    c = _Call("v2_expected_cost", lg.device, out, check)
    risk = c.buf("risk", (B,))
    loss = c.buf("loss", (B,))
    gl = c.buf("grad_logits", (B, T, D), want=need_grad)
    gc = c.buf("grad_cost", (B, T, D), want=need_grad)
    c.workspace(lib.ssnt_v2_expected_cost_workspace_size, B, T, mt, bool(test_mode), bool(need_grad))
    return c.run(lib.ssnt_v2_expected_cost_device, lg.data_ptr(), cs.data_ptr(), table.data_ptr(),
                 il.data_ptr(), ol.data_ptr(), B, T, D, mt, int(zero_duration_id), bool(allow_skip),
                 bool(test_mode), risk, loss, gl, gc)


class V2ExpectedCost(torch.autograd.Function):
    """Autograd wrapper of v2_expected_cost: per-utterance risk (B,), differentiable with respect
    to logits and cost; the gradients come from the same call. The status word is checked in
    backward, as V2DurationLoss does (check=False skips it)."""

    @staticmethod
    def forward(ctx, logits, cost, duration_table, input_length, output_length, zero_duration_id,
                allow_skip=False, test_mode=False, max_total=None, check=True):
        r = v2_expected_cost(logits.detach(), cost.detach(), duration_table, input_length,
                             output_length, zero_duration_id, allow_skip=allow_skip,
                             test_mode=test_mode, max_total=max_total,
                             need_grad=logits.requires_grad or cost.requires_grad)
        ctx.save_for_backward(r.get("grad_logits"), r.get("grad_cost"), r["status"])
        ctx.check = check
        return r["risk"]

    @staticmethod
    def backward(ctx, grad_risk):
        gl, gc, st = ctx.saved_tensors
        if ctx.check:
            _finish("v2_expected_cost_loss", 0, st, True)
        gr = grad_risk.to(torch.float32)[:, None, None]
        need_l, need_c = ctx.needs_input_grad[:2]
        dl = gl * gr if need_l and gl is not None else None
        dc = gc * gr if need_c and gc is not None else None
        return dl, dc, None, None, None, None, None, None, None, None


def v2_expected_cost_loss(logits, cost, duration_table, input_length, output_length,
                          zero_duration_id, allow_skip=False, test_mode=False, max_total=None,
                          check=True):
    """risk (B,) of ``v2_expected_cost``, differentiable in ``logits`` and ``cost`` (minimum-risk
    training on durations, the expected final total in test mode)."""
    return V2ExpectedCost.apply(logits, cost, duration_table, input_length, output_length,
                                zero_duration_id, allow_skip, test_mode, max_total, check)


def v2_duration_entropy(logits, duration_table, input_length, output_length, zero_duration_id,
                        allow_skip=False, test_mode=False, max_total=None, check=True):
    """The entropy H (B,) of the posterior over admissible duration-class sequences,
    differentiable: H = ln Z - E[ln w(path)], with ln Z = -loss of ``v2_duration_loss`` and
    E[ln w] = risk of ``v2_expected_cost_loss`` for cost = logits (a class whose logit is -inf
    has weight zero, so its cost never counts). An utterance without an admissible path gets
    -inf."""
    cost = logits.to(torch.float32)
    loss = v2_duration_loss(logits, duration_table, input_length, output_length, zero_duration_id,
                            allow_skip, test_mode, max_total, False, check)
    risk = v2_expected_cost_loss(logits, cost, duration_table, input_length, output_length,
                                 zero_duration_id, allow_skip, test_mode, max_total, check)
    return -loss - risk


def lattice_beam_search_decode(lattice, input_length, beam_width, *, check=True):
    """Fused T-step v1 beam search over a (B,T,U,2) log-prob lattice: step s feeds every beam
    h = lattice[b, u, t, :] and runs the exact src/lib.rs:121-230 step; then the best final
    beam is backtraced (src/util.rs:20-33, t_history = next_t). Returns a dict of (B,T,W)
    per-step outputs plus best_beam_branch / best_t_history (B,T)."""
    lib = load(require_gpu=True)
    lat = _dev(lattice, torch.float32, "lattice")
    dev = lat.device
    B, T, U, two = lat.shape
    il = _dev(input_length, torch.int32, "input_length").reshape(B)
    W = int(beam_width)
    o = {k: torch.empty((B, T, W), dtype=dt, device=dev) for k, dt in (
        ("prediction", torch.int32), ("log_prob", torch.float32), ("next_t", torch.int32),
        ("next_u", torch.int32), ("next_is_finished", torch.bool), ("beam_branch", torch.int32))}
    o["best_beam_branch"] = torch.empty((B, T), dtype=torch.int32, device=dev)
    o["best_t_history"] = torch.empty((B, T), dtype=torch.int32, device=dev)
    st = _status(dev)
    rc = lib.ssnt_lattice_beam_search_decode_device(
        _p(lat), _p(il), B, T, U, W, _p(o["prediction"]), _p(o["log_prob"]), _p(o["next_t"]),
        _p(o["next_u"]), _p(o["next_is_finished"]), _p(o["beam_branch"]),
        _p(o["best_beam_branch"]), _p(o["best_t_history"]), _p(st), _stream(dev))
    _finish("lattice_beam_search_decode", rc, st, check)
    return o


_STEP_OUTS = (("prediction", torch.int32), ("log_prob", torch.float32), ("next_t", torch.int32),
              ("next_u", torch.int32), ("next_is_finished", torch.bool))


def v2_lattice_beam_search_decode(logits, duration_table, input_length, output_length,
                                  beam_width, zero_duration_id, allow_skip, test_mode, *,
                                  upsample=False, out_of_range_source_index=-1, check=True):
    """Fused multi-step v2 decode over per-step logits (B,T,W,D): every beam starts at
    t = u = 0, log-prob 0, total 0; step s runs the ssnt_tts_v2_beam_search_decode step
    (src/v2.rs:221-339) on h = logits[:, s] and feeds its outputs back as the next state, all in
    one launch. Returns the per-step outputs (B,T,W) under the reference op's output names,
    plus ordered_beam_branch / path_prediction / duration (B,W,T) of every final slot
    (src/v2_util.rs:6-36). upsample=True adds upsampled_source_indexes (B,W,max total) from the
    durations and each slot's final total (src/v2_util.rs:39-66)."""
    lib = load(require_gpu=True)
    lg = _dev(logits, torch.float32, "logits")
    dev = lg.device
    B, T, W, D = lg.shape
    if W != beam_width:
        raise ValueError("logits must be (B, T, beam_width, duration_class_size)")
    table = _dev(duration_table, torch.int32, "duration_table").reshape(D)
    il = _dev(input_length, torch.int32, "input_length").reshape(B)
    # the reference wrapper zeroes output_length in test mode (__init__.py:47)
    ol = torch.zeros_like(il) if test_mode else _dev(output_length, torch.int32,
                                                     "output_length").reshape(B)
    o = {k: torch.empty((B, T, W), dtype=dt, device=dev) for k, dt in _STEP_OUTS}
    o["next_total_duration"] = torch.empty((B, T, W), dtype=torch.int32, device=dev)
    o["beam_branch"] = torch.empty((B, T, W), dtype=torch.int32, device=dev)
    for k in ("ordered_beam_branch", "path_prediction", "duration"):
        o[k] = torch.empty((B, W, T), dtype=torch.int32, device=dev)
    st = _status(dev)
    rc = lib.ssnt_v2_lattice_beam_search_decode_device(
        _p(lg), _p(table), _p(il), _p(ol), B, T, W, D, int(zero_duration_id), bool(allow_skip),
        bool(test_mode), _p(o["prediction"]), _p(o["log_prob"]), _p(o["next_t"]), _p(o["next_u"]),
        _p(o["next_is_finished"]), _p(o["next_total_duration"]), _p(o["beam_branch"]),
        _p(o["ordered_beam_branch"]), _p(o["path_prediction"]), _p(o["duration"]), _p(st),
        _stream(dev))
    _finish("v2_lattice_beam_search_decode", rc, st, check)
    if upsample:
        o["upsampled_source_indexes"] = upsample_source_indexes(
            o["duration"], o["next_total_duration"][:, -1, :], out_of_range_source_index, W,
            check=check)
    return o


def tone_latent_lattice_beam_search_decode(logits, input_length, beam_width, empty_tone_id, *,
                                           check=True):
    """Fused multi-step tone-latent decode over per-step logits (B,T,W,C): the
    tone_latent_beam_search_decode step (src/tone_latent.rs:144-234) T times in one launch.
    Returns the per-step outputs (B,T,W) plus ordered_beam_branch / path_prediction (B,W,T)."""
    lib = load(require_gpu=True)
    lg = _dev(logits, torch.float32, "logits")
    dev = lg.device
    B, T, W, C = lg.shape
    if W != beam_width:
        raise ValueError("logits must be (B, T, beam_width, tone_class_size)")
    il = _dev(input_length, torch.int32, "input_length").reshape(B)
    o = {k: torch.empty((B, T, W), dtype=dt, device=dev) for k, dt in _STEP_OUTS}
    o["beam_branch"] = torch.empty((B, T, W), dtype=torch.int32, device=dev)
    for k in ("ordered_beam_branch", "path_prediction"):
        o[k] = torch.empty((B, W, T), dtype=torch.int32, device=dev)
    st = _status(dev)
    rc = lib.ssnt_tone_latent_lattice_beam_search_decode_device(
        _p(lg), _p(il), B, T, W, C, int(empty_tone_id), _p(o["prediction"]), _p(o["log_prob"]),
        _p(o["next_t"]), _p(o["next_u"]), _p(o["next_is_finished"]), _p(o["beam_branch"]),
        _p(o["ordered_beam_branch"]), _p(o["path_prediction"]), _p(st), _stream(dev))
    _finish("tone_latent_lattice_beam_search_decode", rc, st, check)
    return o
