"""The inputs of the posterior-sampling tests, shared by the CPU reference test (which checks the
share of unclear samples the GPU test relies on) and the GPU test (tests/test_gpu_sample_align.py).
Every case is built and its float64 reference computed once per process. Test infrastructure only."""
import functools

import numpy as np

import sample_ref as SR
import value_cases as VC

LANE_WIDTHS = [1, 2, 63, 64, 65, 127, 128, 129, 256, 257, 512, 513, 1024]
CHUNK_STEPS = [31, 32, 33, 64, 65, 97]
K_EDGES = [1, 2, 63, 64]
TINY = [(obs, terminal) for obs in (False, True) for terminal in (False, True)]
SWITCH_U, SWITCH_K = 80, 16  # the LDS-to-workspace switch is looked for along T at this width


def lattice(B, T, U, seed, obs=False):
    """log_softmax(N(0, 1.5^2)) transitions; log_obs = N(-1, 1) when asked."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((B, T, U, 2)).astype(np.float32) * np.float32(1.5)
    lt = (z - np.logaddexp(z[..., :1], z[..., 1:])).astype(np.float32)
    lo = (rng.standard_normal((B, T, U)) - 1).astype(np.float32) if obs else None
    return lt, lo


def uniforms(B, K, T, seed):
    return np.random.default_rng(1000 + seed).random((B, K, T), dtype=np.float32)


def _case(lt, lo, S, P, K, seed, terminal=True, u=None):
    B, T = lt.shape[:2]
    S, P = np.asarray(S, np.int32), np.asarray(P, np.int32)
    u = uniforms(B, K, T, seed) if u is None else u
    ref = SR.sample_batch(lt, S, P, u, lo)
    ref["clear"] = SR.clear(ref["margin"], ref["feasible"])
    return {"lt": lt, "lo": lo, "S": S, "P": P, "K": K, "u": u, "terminal": terminal, "ref": ref}


@functools.lru_cache(maxsize=None)
def tiny(obs, terminal):
    T, U = 7, 5
    SP = [(S, P) for S in range(0, T + 1) for P in range(0, U + 1)]
    lt, lo = lattice(len(SP), T, U, 11 + 2 * obs + terminal, obs)
    return _case(lt, lo, [s for s, _ in SP], [p for _, p in SP], 3, 1, terminal)


@functools.lru_cache(maxsize=None)
def lane(U):
    B, T = 2, U + 6
    lt, lo = lattice(B, T, U, U, obs=(U % 2 == 1))
    return _case(lt, lo, [T, T - 3], [U, max(1, (2 * U) // 3)], 16, U)


@functools.lru_cache(maxsize=None)
def chunk(T):
    lt, lo = lattice(2, T, 9, T, obs=(T % 2 == 0))
    return _case(lt, lo, [T, T - 1], [9, 5], 16, T)


@functools.lru_cache(maxsize=None)
def k_edge(K):
    lt, lo = lattice(4, 40, 17, 40, obs=True)
    return _case(lt, lo, [40, 33, 17, 25], [17, 9, 17, 1], K, K)


@functools.lru_cache(maxsize=None)
def single_long_row():
    """One sample per utterance on a row of more than 256 positions: the kernel form in which the
    chain wave takes the decisions itself (every other case runs the helper-wave form)."""
    B, T, U = 32, 306, 300
    lt, lo = lattice(B, T, U, 300, obs=True)
    return _case(lt, lo, [T - b % 5 for b in range(B)], [U - 3 * (b % 7) for b in range(B)], 1, 300)


@functools.lru_cache(maxsize=None)
def switch(T):
    lt, lo = lattice(2, T, SWITCH_U, T, obs=True)
    return _case(lt, lo, [T, T - 9], [SWITCH_U, SWITCH_U - 29], SWITCH_K, T)


def switch_T(lib):
    """The largest T whose decision bits stay in LDS at (SWITCH_U, SWITCH_K), by the size query
    (host code only: no GPU call)."""
    q = lambda T: lib.ssnt_sample_align_workspace_size(2, T, SWITCH_U, SWITCH_K)  # noqa: E731
    lo, hi = 1, 1 << 16
    assert q(lo) == 0 and q(hi) > 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if q(mid) == 0 else (lo, mid)
    return lo


@functools.lru_cache(maxsize=None)
def exponent_range():
    B, T, U = 2, 2000, 400
    lt, _ = lattice(B, T, U, T + U)
    return _case(lt, None, [T, T - 37], [U, U - 11], 2, 5)


@functools.lru_cache(maxsize=None)
def zero_probability():
    B, T, U = 16, 12, 5
    rng = np.random.default_rng(0)
    lt, _ = lattice(B, T, U, 1)
    lt[rng.random((B, T, U, 2)) < 0.2] = -np.inf
    lt[0, 3] = -np.inf  # nothing leaves step 3 of utterance 0: infeasible
    S = rng.integers(6, T + 1, size=B)
    S[0] = T
    P = np.array([rng.integers(1, min(s, U) + 1) for s in S])
    return _case(lt, None, S, P, 4, 3)


@functools.lru_cache(maxsize=None)
def frequency():
    B, T, U = 128, 7, 3
    lt1, lo1 = lattice(1, T, U, 21, obs=True)
    lt, lo = np.repeat(lt1, B, axis=0), np.repeat(lo1, B, axis=0)
    return _case(lt, lo, [T] * B, [U] * B, 64, 21)


@functools.lru_cache(maxsize=None)
def reuse():
    lt, lo = lattice(5, 40, 70, 12, obs=True)
    return _case(lt, lo, [40, 33, 40, 12, 25], [40, 20, 1, 12, 25], 8, 12)


@functools.lru_cache(maxsize=None)
def value(name):
    """One input value class of tests/value_cases.py (its TOLERANCE_CLASSES) at B=4, T=48, U=20 with
    16 samples: ragged lengths, S mod 4 = 0, 3, 2, 1. The float64 reference does not depend on the
    distribution; tests/test_value_cases_ref.py holds every case to the cap on the CPU."""
    B, T, U = 4, 48, 20
    lt, _ = lattice(B, T, U, 48)
    S, _ = VC.lengths(B, T, U)
    return _case(VC.lattice(name, lt), None, S, [20, 13, 7, 12], 16, 7)


def capped(lib):
    """(name, case) of every case whose unclear share the GPU test holds to the cap."""
    Tl = switch_T(lib)
    out = [(f"tiny{o}{t}", tiny(o, t)) for o, t in TINY]
    out += [(f"lane{U}", lane(U)) for U in LANE_WIDTHS]
    out += [(f"chunk{T}", chunk(T)) for T in CHUNK_STEPS]
    out += [(f"k{K}", k_edge(K)) for K in K_EDGES]
    out += [(f"switch{T}", switch(T)) for T in (Tl, Tl + 1)]
    out += [("single long row", single_long_row())]
    out += [("zero", zero_probability()), ("frequency", frequency()), ("reuse", reuse())]
    out += [(f"value {n}", value(n)) for n in VC.TOLERANCE_CLASSES]
    return out


CAP_CASE, CAP_ALL = 0.25, 0.05


def unclear_share(case):
    """(unclear, total) over the feasible utterances' samples."""
    f = case["ref"]["feasible"]
    n = int(f.sum()) * case["K"]
    return n - int(case["ref"]["clear"].sum()), n
