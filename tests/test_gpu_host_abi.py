"""The host-pointer C ABI (csrc/capi.hip) as the TF ops use it: every staging plan of every
reference symbol and of ssnt_fwd_bwd, one per-thread context through growing and shrinking
calls, optional outputs, error returns that leave no trace, concurrent callers, and the release
of a context when its thread exits. Every result is bit-exact against the C oracle.

The staging plan of a call ("zero-copy" up to 1 MiB, one H2D / D2H "copy" above it, "direct"
copies of the caller's arrays from 8 MiB of log_trans) is read from the A/B build's
ssnt_diag_host_path at default knobs; the same call is checked on the product library as well.
All oracle references are computed on the main thread, before any worker thread starts."""
import ctypes
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest
import torch

import host_abi_cases as hc
from gpu_util import _t

pytestmark = pytest.mark.gpu

OK, INVALID_ARG, BAD_LENGTH = 0, 1, 7
FLAGS = 1 | 2  # terminal emit, zero_infinity


def host_path(ab):
    buf = ctypes.create_string_buffer(32)
    ab.ssnt_diag_host_path(buf, 32)
    return buf.value.decode()


def on_both(gpu, fn):
    """fn(None) on the product library, then fn(ab) inside use_ab() at default knobs."""
    fn(None)
    with gpu.use_ab() as ab:
        fn(ab)


def in_thread(fn, limit=120.0):
    """Run fn() in a fresh thread (an empty host context) and return what it returned."""
    box = {}

    def body():
        try:
            box["value"] = fn()
        except BaseException as e:  # noqa: BLE001  (an assertion raised in a thread would be lost)
            box["error"] = repr(e)
    th = threading.Thread(target=body)
    th.start()
    th.join(limit)
    assert not th.is_alive(), "the thread did not finish"
    assert "error" not in box, box["error"]
    return box["value"]


# ---- a. every plan, every symbol ---------------------------------------------------------------
# ssnt_tts_beam_search_decode has batch 1 and 42 bytes per beam: its beam width is bounded by the
# step kernel's LDS (3200 candidates, W <= 1600: 67 KB) long before a plan reaches 1 MiB, so it has
# the zero-copy case only.
PLAN_CASES = {
    "v1-small": lambda o: hc.v1_step(o, 3, W=8),
    "v2-small": lambda o: hc.v2_step(o, 0),
    "v2-large": lambda o: hc.v2_step_sized(o, 0, B=256, W=8, D=128),
    "tone-small": lambda o: hc.tone_step(o, 1),
    "tone-large": lambda o: hc.tone_step(o, 0, B=256, W=8, C=128),
    "order-small": lambda o: hc.order(o, 3, 4, 50),
    "order-large": lambda o: hc.order(o, 8, 4, 9000),
    "upsample-small": lambda o: hc.upsample(o, 2, 3, 20, 130),
    "upsample-large": lambda o: hc.upsample(o, 2, 4, 400, 40000),
    "edit-small": lambda o: hc.edit_distance(o, 5, 40),
    "edit-large": lambda o: hc.edit_distance(o, 48, 3000),
    "extract-small": lambda o: hc.extract(o, 4, 60),
    "extract-large": lambda o: hc.extract(o, 4, 40000),
}


@pytest.mark.parametrize("name", list(PLAN_CASES))
def test_every_plan_every_symbol(gpu, oracle, name):
    from ssnt_tts_amd import capi
    case = PLAN_CASES[name](oracle)
    large = name.endswith("-large")
    # well under the line, or over it
    assert case.plan_bytes > hc.MIB if large else case.plan_bytes < hc.MIB // 4, case.plan_bytes

    def check(ab):
        bad = case.run(capi)
        assert bad is None, ("product" if ab is None else "A/B", bad)
        if ab is not None:
            assert host_path(ab) == ("copy" if large else "zero-copy"), case.name
    on_both(gpu, check)


@pytest.mark.ab
@pytest.mark.parametrize("name", [n for n in PLAN_CASES if n.endswith("-small")])
def test_small_plans_with_copies(gpu, oracle, name):
    # ssnt_set_host_staging(0): the small plans through the H2D / D2H copies
    from ssnt_tts_amd import capi
    case = PLAN_CASES[name](oracle)
    with gpu.use_ab() as ab:
        assert ab.ssnt_set_host_staging(0) == 1
        bad = case.run(capi)
        assert bad is None, bad
        assert host_path(ab) == "copy"


# ---- the forward-backward at the 8 MiB switch (shared by b, c, d, e) ---------------------------
class Switch:
    """(64, 128, 128): exactly 8 MiB of log_trans, the first direct plan; its first 63 utterances
    are the last copied one. log_obs, ragged lengths, utterance 7 infeasible (zero_infinity)."""
    T, U = 128, 128

    def __init__(self, oracle):
        self.lt, self.lo, self.S, self.P = hc.lattice_inputs(oracle, 64, self.T, self.U, seed=21,
                                                             infeasible=7)
        assert self.lt[:64].nbytes == 8 * hc.MIB and self.lt[:63].nbytes < 8 * hc.MIB
        self.want = oracle.fwd_bwd_xf(self.lt, self.S, self.P, log_obs=self.lo, flags=FLAGS,
                                      debug=True)
        assert self.want["loss"][7] == 0.0 and not self.want["grad"][7].any()
        assert np.isfinite(self.want["loss"]).all() and (np.delete(self.want["loss"], 7) > 0).all()

    def outputs(self, B, keys, fill=0x5A):
        out = {k: None for k in hc.FB_KEYS}
        for k in keys:
            out[k] = np.full(self.want[k][:B].shape, 0, np.float32)
            out[k].view(np.uint8)[...] = fill
        return out

    def call(self, capi, B, keys, lt=None, out=None, obs=True):
        """One raw call on the first B utterances; returns (status, the output dict)."""
        out = self.outputs(B, keys) if out is None else out
        rc = capi.ssnt_fwd_bwd_raw(self.lt[:B] if lt is None else lt, self.lo[:B] if obs else None,
                                   self.S[:B], self.P[:B], B, self.T, self.U, FLAGS,
                                   *[out[k] for k in hc.FB_KEYS])
        return rc, out

    def mismatch(self, B, out):
        for k, v in out.items():
            if v is not None and not hc.same(v, self.want[k][:B]):
                return f"{k} differs from the oracle (B={B})"
        return None


@pytest.fixture(scope="module")
def switch(oracle):
    return Switch(oracle)


SIDES = [pytest.param(64, "direct", id="8MiB-direct"), pytest.param(63, "copy", id="below-copy")]


# ---- c. ssnt_fwd_bwd at the 8 MiB switch --------------------------------------------------------
@pytest.mark.parametrize("B,path", SIDES)
def test_fwd_bwd_at_the_switch(gpu, switch, B, path):
    from ssnt_tts_amd import capi
    subsets = [hc.FB_KEYS,                                    # all five outputs
               ("loss",),                                     # grad_trans NULL: the loss only
               ("loss", "grad"),                              # grad_obs NULL while log_obs is given
               ("loss", "grad", "grad_obs", "log_alpha"),     # exactly one of log_alpha / log_beta
               ("loss", "grad", "grad_obs", "log_beta")]

    def check(ab):
        for keys in subsets:
            rc, out = switch.call(capi, B, keys)
            assert rc == OK, (keys, rc)
            assert switch.mismatch(B, out) is None, (keys, switch.mismatch(B, out))
            if ab is not None:
                assert host_path(ab) == path, keys
        # log_trans and grad 4 bytes into larger host arrays
        n = B * switch.T * switch.U * 2
        big_in, big_out = np.empty(n + 3, np.float32), np.full(n + 3, 7.5, np.float32)
        lt = big_in[1:1 + n].reshape(B, switch.T, switch.U, 2)
        lt[...] = switch.lt[:B]
        out = switch.outputs(B, ("loss", "grad_obs"))
        out["grad"] = big_out[1:1 + n].reshape(lt.shape)
        assert lt.ctypes.data % 8 == 4 and out["grad"].ctypes.data % 8 == 4
        rc, out = switch.call(capi, B, None, lt=lt, out=out)
        assert rc == OK and switch.mismatch(B, out) is None, (rc, switch.mismatch(B, out))
        assert big_out[0] == 7.5 and (big_out[1 + n:] == 7.5).all()  # nothing beside the view
        if ab is not None:
            assert host_path(ab) == path
    on_both(gpu, check)


# ---- d. errors leave no trace -------------------------------------------------------------------
def _untouched(out):
    return all((v.view(np.uint8) == 0x5A).all() for v in out.values() if v is not None)


@pytest.mark.parametrize("B,path", SIDES)
def test_errors_leave_no_trace(gpu, switch, B, path):
    # Every output, the loss included, is filled with 0x5A bytes; a refused or failed call must
    # leave every one of them, in the staged plan and in the direct one (where the status word is
    # read before any output is copied back); the next valid call on the thread is bit-exact.
    from ssnt_tts_amd import capi
    sw, T, U = switch, switch.T, switch.U
    lt, lo = sw.lt[:B], sw.lo[:B]

    def check(ab):
        out = sw.outputs(B, hc.FB_KEYS)
        o5 = [out[k] for k in hc.FB_KEYS]
        S, P = sw.S[:B].copy(), sw.P[:B].copy()
        bad = S.copy()
        bad[B - 2] = T + 1  # a length beyond the tensor, found by the kernel
        raw = capi.ssnt_fwd_bwd_raw
        assert raw(lt, lo, bad, P, B, T, U, FLAGS, *o5) == BAD_LENGTH
        if ab is not None:
            assert host_path(ab) == path  # the plan the failed call went through
        assert _untouched(out), "SSNT_ERR_BAD_LENGTH wrote an output"
        refused = {
            "log_trans NULL": (None, lo, S, P, B, T, U, FLAGS, *o5),
            "step_len NULL": (lt, lo, None, P, B, T, U, FLAGS, *o5),
            "loss NULL": (lt, lo, S, P, B, T, U, FLAGS, None, *o5[1:]),
            "grad_obs without log_obs": (lt, None, S, P, B, T, U, FLAGS, *o5),
            "max_steps 0": (lt, lo, S, P, B, 0, U, FLAGS, *o5),
            "max_steps -1": (lt, lo, S, P, B, -1, U, FLAGS, *o5),
        }
        for what, args in refused.items():
            assert raw(*args) == INVALID_ARG, what
            assert _untouched(out), what
        assert raw(lt, lo, S, P, 0, T, U, FLAGS, *o5) == OK  # an empty batch
        assert _untouched(out), "batch 0 wrote an output"
        rc, out = sw.call(capi, B, hc.FB_KEYS, out=out)
        assert rc == OK and sw.mismatch(B, out) is None, (rc, sw.mismatch(B, out))
        if ab is not None:
            assert host_path(ab) == path
    on_both(gpu, check)


# ---- b. one context through a growth sequence ---------------------------------------------------
def test_one_context_grows_and_shrinks(gpu, oracle, switch):
    # a fresh thread, so the context starts empty: its pinned buffer and device scratch are
    # reallocated on the way up (ensure() frees, the mapped address is looked up again) and
    # reused, larger than needed, on the way down
    from ssnt_tts_amd import capi
    direct = hc.Case("fwd_bwd direct", lambda c: _switch_outputs(switch, c, 64),
                     [switch.want[k] for k in hc.FB_KEYS], switch.lt.nbytes)
    steps = [(hc.v1_step(oracle, 1, W=4), "zero-copy"),
             (hc.order(oracle, 8, 4, 9000), "copy"),
             (hc.v2_step(oracle, 2), "zero-copy"),
             (hc.fwd_bwd(oracle, 3, 40, 20, seed=2), "copy"),
             (direct, "direct"),
             (hc.v1_step(oracle, 6, W=3), "zero-copy"),
             (hc.upsample(oracle, 2, 4, 400, 40000), "copy")]
    assert steps[0][0].plan_bytes < 1024 and steps[3][0].plan_bytes < hc.MIB

    def sequence(ab):
        bad = []
        for i, (case, path) in enumerate(steps):
            r = case.run(capi)
            if r is not None:
                bad.append(f"step {i + 1}: {r}")
            if ab is not None and host_path(ab) != path:
                bad.append(f"step {i + 1} {case.name}: plan {host_path(ab)!r}, expected {path!r}")
        return bad

    def check(ab):
        assert in_thread(lambda: sequence(ab)) == []
    on_both(gpu, check)


def _switch_outputs(switch, capi, B):
    rc, out = switch.call(capi, B, hc.FB_KEYS)
    assert rc == OK
    return [out[k] for k in hc.FB_KEYS]


# ---- e. threads ---------------------------------------------------------------------------------
def test_concurrent_host_callers(gpu, oracle, switch):
    # Four threads call the product library at once (ctypes releases the GIL for the call), each
    # on its own thread-local context, while the main thread keeps device entries busy on a torch
    # stream of its own. Batches stay small, so the kernels of all threads fit the chip together.
    from ssnt_tts_amd import capi
    NW, ROUNDS = 4, 40
    rotation = [hc.v1_step(oracle, 1, W=1), hc.v1_step(oracle, 2, W=5), hc.v1_step(oracle, 4, W=8),
                hc.v2_step(oracle, 0), hc.v2_step(oracle, 9), hc.tone_step(oracle, 1),
                hc.tone_step(oracle, 7), hc.order(oracle, 2, 3, 33), hc.upsample(oracle, 2, 2, 30, 170),
                hc.edit_distance(oracle, 3, 70), hc.extract(oracle, 5, 90),
                hc.fwd_bwd(oracle, 3, 24, 12, seed=3)]
    stream_case = hc.fwd_bwd(oracle, 2, 30, 80, seed=4, obs=False, debug=False)   # streaming kernel
    wide_case = hc.fwd_bwd(oracle, 2, 20, 257, seed=5, obs=False, debug=False)    # long-row kernel
    direct = hc.Case("fwd_bwd direct", lambda c: _switch_outputs(switch, c, 64),
                     [switch.want[k] for k in hc.FB_KEYS], switch.lt.nbytes)
    own = {1: (stream_case, "k_fwd_bwd_stream<"), 2: (wide_case, "k_fwd_bwd_wide<")}

    # the main thread's device calls and their references
    lt, lo, S, P = hc.lattice_inputs(oracle, 3, 50, 20, seed=6)
    want_fb = oracle.fwd_bwd_xf(lt, S, P, log_obs=lo)
    from f4_cases import random_case
    logits, I, O = random_case(np.random.default_rng(8), 3, 9, 5)
    table = np.arange(5, dtype=np.int32)
    want_v2 = oracle.v2_fwd_bwd(logits, table, I, O, int(O.max()), 0, True, False)
    dev_fb = [_t(x) for x in (lt, S, P, lo)]
    dev_v2 = [_t(x) for x in (logits, table, I, O)]

    mismatches, stop, barrier = [], threading.Event(), threading.Barrier(NW)

    def worker(w):
        try:
            barrier.wait(30)
            for r in range(ROUNDS):
                for j in range(len(rotation)):
                    if stop.is_set():
                        return
                    bad = rotation[(j + 3 * w) % len(rotation)].run(capi)
                    if bad:
                        raise AssertionError(bad)
                if w in own:
                    case, kernel = own[w]
                    bad = case.run(capi)
                    k = gpu.last_fwd_bwd_kernel()
                    if bad or not k.startswith(kernel):
                        raise AssertionError(bad or f"{case.name}: this thread's last kernel reads {k}")
                if w == 0 and r == ROUNDS // 2:
                    bad = direct.run(capi)
                    if bad:
                        raise AssertionError(bad)
        except BaseException as e:  # noqa: BLE001
            mismatches.append(f"worker {w}: {e!r}")
            stop.set()

    threads = [threading.Thread(target=worker, args=(w,)) for w in range(NW)]
    for th in threads:
        th.start()
    side, n_dev = torch.cuda.Stream(), 0
    with torch.cuda.stream(side):
        while any(th.is_alive() for th in threads) and not stop.is_set() and n_dev < 2000:
            g = gpu.ssnt_fwd_bwd(dev_fb[0], dev_fb[1], dev_fb[2], dev_fb[3], check=True)
            v = gpu.v2_fwd_bwd(dev_v2[0], dev_v2[1], dev_v2[2], dev_v2[3], 0, allow_skip=True,
                               max_total=int(O.max()), check=True)
            for k in ("loss", "grad", "grad_obs"):
                if not hc.same(g[k].cpu().numpy(), want_fb[k]):
                    mismatches.append(f"main: ssnt_fwd_bwd {k} (call {n_dev})")
            for k in ("loss", "grad"):
                if not hc.same(v[k].cpu().numpy(), want_v2[k]):
                    mismatches.append(f"main: v2_fwd_bwd {k} (call {n_dev})")
            if mismatches:
                stop.set()
            n_dev += 1
    for th in threads:
        th.join(120)
    alive = [i for i, th in enumerate(threads) if th.is_alive()]
    if alive:
        stop.set()
    assert not alive, f"workers still running after 120 s: {alive}"
    assert mismatches == []
    assert n_dev > 0


# ---- f. thread lifetime -------------------------------------------------------------------------
def test_context_is_released_when_its_thread_exits(gpu, oracle):
    from ssnt_tts_amd import capi
    N = 8
    case = hc.v1_step(oracle, 1, W=4)
    with gpu.use_ab() as ab:
        assert case.run(capi) is None  # the main thread's own context exists from here on
        before = ab.ssnt_diag_host_contexts()
        assert before >= 1
        called, leave, bad = threading.Barrier(N + 1), threading.Event(), []

        def body():
            try:
                r = case.run(capi)
                if r:
                    bad.append(r)
            except BaseException as e:  # noqa: BLE001
                bad.append(repr(e))
            called.wait(60)
            leave.wait(60)
        threads = [threading.Thread(target=body) for _ in range(N)]
        for th in threads:
            th.start()
        try:
            called.wait(60)  # every thread has made its call and is parked
            during = ab.ssnt_diag_host_contexts()
        finally:
            leave.set()
            for th in threads:
                th.join(60)
        assert not any(th.is_alive() for th in threads) and bad == []
        assert during == before + N
        # join() returns when a thread's Python state is gone; its thread-local destructors run
        # at the end of the OS thread, a moment later: poll, with a bound
        deadline = time.monotonic() + 10.0
        while ab.ssnt_diag_host_contexts() != before and time.monotonic() < deadline:
            time.sleep(0.001)
        assert ab.ssnt_diag_host_contexts() == before
        assert case.run(capi) is None  # and the main thread's context still works


def test_process_exits_cleanly_after_host_calls(gpu):
    # the main thread's context is released by its thread-local destructor at process exit, after
    # two worker threads' contexts were released at their exits: the process must end with status
    # 0 and its last line printed
    root = os.path.join(os.path.dirname(__file__), "..")
    code = r"""
import sys, threading
import numpy as np
sys.path.insert(0, %r)
from ssnt_tts_amd import capi
def call():
    W = 3
    out = capi.ssnt_tts_beam_search_decode(np.zeros((W, 2), np.float32), np.zeros(W, np.float32),
                                           np.zeros(W, bool), np.zeros(W, np.int32),
                                           np.zeros(W, np.int32), 4, W)
    assert out[0].shape == (W,)
call()
for _ in range(2):
    th = threading.Thread(target=call)
    th.start()
    th.join()
call()
print("last line", flush=True)
""" % os.path.join(root, "ssnt-tts-rust_amd")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert r.stdout.strip().splitlines()[-1] == "last line", r.stdout
