"""Dirtying helpers of the contract tests: overwrite every input cell a lattice
call's contract never reads with a value that shows in the result if it is read after all -- even
as 0 * x. Pure numpy; the CPU references are held to the same property in
tests/test_contract_ref.py, and the GPU tests (tests/test_gpu_contract.py) cover exactly the cell
classes that pass there. Test infrastructure only."""
import numpy as np


def _f32(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


# -inf is not among them: it is what the masks produce anyway
VALUES = {
    "nan": _f32(0x7FC00000),        # the default quiet NaN
    "nan_ones": _f32(0xFFFFFFFF),   # the all-ones pattern (what a 0xFF fill leaves)
    "inf": np.float32(np.inf),
    "1e30": np.float32(1e30),
    "88": np.float32(88.0),         # exp(88) sits at the edge of the f32 range
}
ALTERNATING = ("inf", "1e30", "88")  # run C of the GPU tests: one of these per utterance, in turn


def alternating(B):
    return np.array([VALUES[ALTERNATING[b % 3]] for b in range(B)], np.float32)


def _bits(value, B):
    """`value` (one f32 or one per utterance) as B uint32 patterns: a NaN's payload survives."""
    return np.broadcast_to(np.asarray(value, np.float32).reshape(-1).view(np.uint32), (B,))


def lattice_dead_mask(shape, S, P, terminal):
    """(mask_trans (B,T,U,2), mask_obs (B,T,U)) bool: the cells the emit/shift contract never reads
    with extents S_b, P_b (lengths outside the tensor are clipped to it):
    rows s >= S_b; positions p >= P_b; the shift out of P_b - 1; every shift of row S_b - 1; the
    emits of row S_b - 1 at p != P_b - 1, and at P_b - 1 too without the terminal emit."""
    B, T, U = shape[:3]
    mt = np.zeros((B, T, U, 2), bool)
    mo = np.zeros((B, T, U), bool)
    for b in range(B):
        s, p = int(np.clip(S[b], 0, T)), int(np.clip(P[b], 0, U))
        mt[b, s:], mt[b, :, p:] = True, True
        mo[b, s:], mo[b, :, p:] = True, True
        if p >= 1:
            mt[b, :, p - 1, 1] = True
        if s >= 1:
            mt[b, s - 1, :, 1] = True
            mt[b, s - 1, :, 0] = True
            if p >= 1 and terminal:
                mt[b, s - 1, p - 1, 0] = False
    return mt, mo


def dirty_lattice(lt, lo, S, P, value, terminal):
    """Copies of log_trans (B,T,U,2) and log_obs (B,T,U) or None with every dead cell := value."""
    lt = np.array(lt, np.float32)
    B = lt.shape[0]
    mt, mo = lattice_dead_mask(lt.shape, S, P, terminal)
    bits = _bits(value, B)
    ltb = lt.view(np.uint32)
    ltb[mt] = np.broadcast_to(bits[:, None, None, None], lt.shape)[mt]
    if lo is None:
        return lt, None
    lo = np.array(lo, np.float32)
    lo.view(np.uint32)[mo] = np.broadcast_to(bits[:, None, None], lo.shape)[mo]
    return lt, lo


def v2_dead_mask(shape, I, zid, allow_skip):
    """(B,T,D) bool: logits rows t >= I_b, and column zid when the zero-duration class is barred."""
    B, T, D = shape
    m = np.zeros((B, T, D), bool)
    for b in range(B):
        m[b, int(np.clip(I[b], 0, T)):] = True
    if not allow_skip:
        m[:, :, zid] = True
    return m


def dirty_v2(logits, I, value, zid, allow_skip):
    """A copy of logits (B,T,D) with every dead cell := value."""
    lg = np.array(logits, np.float32)
    m = v2_dead_mask(lg.shape, I, zid, allow_skip)
    lg.view(np.uint32)[m] = np.broadcast_to(_bits(value, lg.shape[0])[:, None, None], lg.shape)[m]
    return lg


def same_bits(a, b):
    """Bit-identical arrays (dicts: every key)."""
    if isinstance(a, dict):
        return set(a) == set(b) and all(same_bits(a[k], b[k]) for k in a)
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
