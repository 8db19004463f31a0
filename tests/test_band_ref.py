"""The definition of the banded forward-backward on the CPU: the oracle on the
embedding agrees with a brute force over the paths inside the band and with an independent float64
DP in band coordinates, gradients outside the band are exact zeros, and the two-block form of Z at
the cut has the oracle's bits. No GPU."""
import numpy as np

import band_ref as BR

F32 = np.float32
KINDS = ("stay", "diag", "alt", "random")


def _inputs(rng, T, R, obs):
    z = rng.standard_normal((1, T, R, 2)).astype(F32) * F32(1.5)
    m = z.max(axis=-1, keepdims=True)
    lt = (z - (m + np.log(np.exp(z - m).sum(axis=-1, keepdims=True)))).astype(F32)
    lo = (rng.standard_normal((1, T, R)) * 3 - 4).astype(F32) if obs else None
    return lt, lo


def _cases(shapes, seed):
    """(lt, lo, bs, S, P, R, terminal) over shapes x band families x with / without log_obs."""
    rng = np.random.default_rng(seed)
    for (T, S, P, R) in shapes:
        for kind in KINDS:
            bs = BR.make_band(kind, T, S, P, R, rng)
            if bs is None:
                continue
            assert BR.is_valid(bs, S, P, R)
            for obs in (False, True):
                lt, lo = _inputs(rng, T, R, obs)
                yield lt, lo, bs[None], S, P, R, bool((T + S + P + obs) % 2)


TINY = [(7, 7, 3, 2), (7, 6, 4, 3), (6, 6, 6, 1), (5, 5, 1, 1), (7, 7, 2, 3), (6, 5, 3, 3), (4, 4, 4, 2),
        (1, 1, 1, 1), (7, 7, 5, 3), (3, 2, 2, 2)]
SMALL = [(12, 12, 5, 4), (20, 17, 9, 8), (24, 24, 24, 4), (30, 30, 20, 16), (16, 13, 1, 4), (21, 21, 12, 5),
         (18, 18, 17, 16), (9, 9, 9, 8), (32, 29, 3, 8), (15, 15, 6, 16)]


def test_oracle_on_the_embedding_is_the_brute_force(oracle):
    n = 0
    for lt, lo, bs, S, P, R, term in _cases(TINY, 1):
        o = BR.oracle_band(oracle, lt, lo, bs, [S], [P], flags=1 if term else 0)
        loss, grad, gobs = BR.brute_force(lt[0], None if lo is None else lo[0], bs[0], S, P, term)
        assert abs(float(o["loss"][0]) - loss) <= 1e-5 + 2.0 ** -23 * abs(loss)
        assert np.abs(o["grad"][0] - grad).max() <= 1e-5
        if lo is not None:
            assert np.abs(o["grad_obs"][0] - gobs).max() <= 1e-5
        n += 1
    assert n >= 40


def test_oracle_on_the_embedding_is_the_float64_band_dp(oracle):
    n = 0
    for lt, lo, bs, S, P, R, term in _cases(SMALL, 2):
        o = BR.oracle_band(oracle, lt, lo, bs, [S], [P], flags=1 if term else 0)
        loss, grad, gobs = BR.band_dp64(lt[0], None if lo is None else lo[0], bs[0], S, P, term)
        assert abs(float(o["loss"][0]) - loss) <= 1e-5 + 2.0 ** -23 * abs(loss)
        assert np.abs(o["grad"][0] - grad).max() <= 1e-5
        if lo is not None:
            assert np.abs(o["grad_obs"][0] - gobs).max() <= 1e-5
        n += 1
    assert n >= 50


def test_band_dp_is_the_brute_force():
    for lt, lo, bs, S, P, R, term in _cases(TINY, 3):
        a = BR.band_dp64(lt[0], None if lo is None else lo[0], bs[0], S, P, term)
        b = BR.brute_force(lt[0], None if lo is None else lo[0], bs[0], S, P, term)
        assert abs(a[0] - b[0]) <= 1e-9 * max(1.0, abs(b[0]))
        assert np.abs(a[1] - b[1]).max() <= 1e-9
        if lo is not None:
            assert np.abs(a[2] - b[2]).max() <= 1e-9


def test_gradients_outside_the_band_are_exact_zeros(oracle):
    for lt, lo, bs, S, P, R, term in _cases(SMALL, 4):
        o = BR.oracle_band(oracle, lt, lo, bs, [S], [P], flags=1 if term else 0)
        U = o["U"]
        inside = np.zeros((1, lt.shape[1], U), bool)
        leaving = np.zeros((1, lt.shape[1], U, 2), bool)
        for s in range(S):
            p0 = int(bs[0, s])
            inside[0, s, p0:p0 + R] = True
            if s + 1 < S:
                if bs[0, s + 1] == p0:
                    if p0 + R - 1 < U:
                        leaving[0, s, p0 + R - 1, 1] = True
                else:
                    leaving[0, s, p0, 0] = True
        for zero in (o["dense_grad"][~inside], o["dense_grad"][leaving]):
            assert not zero.view(np.uint32).any()  # +0, not -0
        if lo is not None:
            assert not o["dense_grad_obs"][~inside].view(np.uint32).any()


def test_two_block_z_has_the_oracles_bits(oracle):
    rng = np.random.default_rng(5)
    n = 0
    for R in (1, 2, 3, 5, 8, 12, 16):
        for _ in range(12):
            S = int(rng.integers(1, 40))
            P = int(rng.integers(1, S + 1))
            T = S + int(rng.integers(0, 3))
            bs = BR.make_band("random", T, S, P, R, rng)
            lt, lo = _inputs(rng, T, R, bool(n % 2))
            dlt, dlo = BR.embed(lt, lo, bs[None], [S], [P])
            st = oracle.fwd_bwd_xf_state(dlt, [S], [P], dlo)
            zm, ze = BR.two_block_z(st["alpha"][0], st["beta"][0], bs, S, P, R)
            assert (F32(zm).tobytes(), int(ze)) == (st["z"]["m"][0].tobytes(), int(st["z"]["e"][0]))
            n += 1
    assert n >= 80
