"""The rounding rule of the compact optimizer step (pipelinerl_amd/csrc/prl_optim_sr.h) compiled for the host with
g++ -ffp-contract=off, on a machine without a GPU: the generator's known answers, stochastic rounding exhaustively over its
random value, the compact update bit for bit against the composition oracle of tests/optim_compact_checks.py, and the two
unbiasedness experiments on that oracle (so that the bound the GPU test applies is known to hold for the reference alone).
The kernel itself is covered by tests/test_gpu_optim_compact.py."""

import ctypes
import subprocess

import numpy as np
import pytest

import optim_compact_checks as cc
from optim_checks import log_uniform_grads

U32 = ctypes.POINTER(ctypes.c_uint32)


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    d = tmp_path_factory.mktemp("compact_harness")
    return cc.build_optmath(d), cc.build_compact(d)


def test_philox_known_answers(libs):
    _, compact = libs
    for counter, key, want in cc.KNOWN_ANSWERS:
        c, k, out = (ctypes.c_uint32 * 4)(*counter), (ctypes.c_uint32 * 2)(*key), (ctypes.c_uint32 * 4)()
        compact.prl_host_philox4x32_10(c, k, out)
        assert tuple(out) == want, f"header: counter {counter} key {key}: {[hex(x) for x in out]}"
        got = cc.philox4x32_10(*counter, *key)
        assert tuple(int(w[0]) for w in got) == want, f"numpy: counter {counter} key {key}"


def test_call_indexing_matches_the_numpy_restatement(libs):
    """Element 4q + j takes word j of the call with counter (q lo, q hi, step, ordinal): header against numpy, over a group
    boundary, a nonzero offset, an index past 2^32 and a 64-bit seed."""
    _, compact = libs
    for off, step, ordinal, seed in ((0, 1, 0, 0), (16, 7, 3, 12345), ((1 << 34) + 4, 2 ** 31 + 5, 2 ** 32 - 1, 2 ** 64 - 1)):
        n = 37
        x = np.zeros(n, np.uint32)
        compact.prl_host_sr_words(n, off, step, ordinal, seed, x.ctypes.data_as(U32))
        want = cc.sr_words(off + np.arange(n), step, ordinal, seed)
        assert np.array_equal(x, want)
        q = (off >> 2) + 1  # the second group, spelled out
        words = cc.philox4x32_10(q & 0xFFFFFFFF, q >> 32, step & 0xFFFFFFFF, ordinal, seed & 0xFFFFFFFF, seed >> 32)
        assert [int(x[4 + j]) for j in range(4)] == [int(w[0]) for w in words]
    # the three 16-bit values: each uniform, pairwise independent (any two determine the word's halves)
    x = cc.sr_words(np.arange(1 << 16), 1, 0, 0)
    for r in (cc.r_p(x), cc.r_m(x), cc.r_v(x)):
        assert r.max() < 65536 and abs(r.astype(np.float64).mean() - 32767.5) < 4 * 65536 / np.sqrt(12 * x.size)
    assert np.array_equal(cc.r_p(x) ^ cc.r_m(x), cc.r_v(x))


SR_VALUES = {  # fp32 bit patterns
    "normal": 0x3F9E0419, "subnormal": 0x00012345, "negative": 0xC0490FDB, "low bits 0": 0x3F800000, "low bits 0xffff": 0x3F80FFFF,
    "just under a power of two": 0x3FFFFFFF, "largest finite bf16": 0x7F7F0000, "above the largest finite bf16": 0x7F7F8000,
    "negative subnormal": 0x80000001,
}


@pytest.mark.parametrize("name", SR_VALUES)
def test_sr_is_exact_over_all_random_values(libs, name):
    _, compact = libs
    u = SR_VALUES[name]
    f = np.array([u], np.uint32).view(np.float32)[0]
    out = np.zeros(65536, np.uint16)
    compact.prl_host_sr_all(f, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)))
    lo, hi = u >> 16, (u >> 16) + 1
    assert np.all((out == lo) | (out == hi)), "every result is one of the two neighbouring bf16 values"
    assert int((out == hi).sum()) == (u & 0xFFFF), "the number of random values that round up equals the low 16 bits: the expectation is the value"
    assert np.all(np.diff(out.astype(np.int32)) >= 0)
    assert np.array_equal(out, cc.sr(np.full(65536, f, np.float32), np.arange(65536))), "numpy restatement"
    if name == "above the largest finite bf16":
        assert out[-1] == 0x7F80, "a finite value above the largest bf16 may become inf, as under round-to-nearest"


def test_sr_special_values(libs):
    _, compact = libs
    for u, want in ((0x7F800000, 0x7F80), (0xFF800000, 0xFF80), (0x00000000, 0x0000), (0x80000000, 0x8000)):
        f = np.array([u], np.uint32).view(np.float32)[0]
        for r in (0, 1, 0x7FFF, 0x8000, 0xFFFF):
            assert compact.prl_host_sr(f, r) == want, (hex(u), r)
    for u in (0x7FC00000, 0x7F800001, 0xFFC12345, 0x7FFFFFFF, 0xFFFFFFFF):
        f = np.array([u], np.uint32).view(np.float32)[0]
        for r in (0, 0xFFFF):
            assert compact.prl_host_sr(f, r) == 0x7FC0, (hex(u), r)
            assert cc.sr(np.array([f]), np.array([r]))[0] == 0x7FC0


N, STEPS = 4099, 5
COEFS = [1.0, 0.37, 1.0, 0.0123, 1.0]  # clip coefficient 1 and < 1


@pytest.mark.parametrize("elem_offset", [0, 16])
@pytest.mark.parametrize("state_bf16", [False, True])
@pytest.mark.parametrize("mode", cc.MODES)
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("rule", ["adamw", "lion"])
def test_compact_update_is_the_composition_of_pinned_parts(libs, rule, wd, mode, state_bf16, elem_offset):
    """Every entry, every stored array, 5 steps: the header's compact update = widen -> prl_host_adamw / prl_host_lion -> numpy sr."""
    optmath, compact = libs
    rng = np.random.default_rng(11)
    lr, betas = (1e-3, (0.9, 0.999)) if rule == "adamw" else (1e-4, (0.9, 0.99))
    seed, ordinal = 0x1234567890ABCDEF, 5
    p0 = rng.normal(0.0, 0.05, N).astype(np.float32)
    if mode != "f32":
        p0 = cc.rne(p0)
    grads = log_uniform_grads(rng, N, STEPS)
    oracle = cc.CompactOracle(optmath, rule, mode, state_bf16, p0, lr=lr, wd=wd, betas=betas, seed=seed, ordinal=ordinal, elem_offset=elem_offset)
    sdt = np.uint16 if state_bf16 else np.float32
    p, m, v = p0.copy(), np.zeros(N, sdt), np.zeros(N, sdt)
    master = cc.widen(p0).copy() if mode == "master" else None
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    for k in range(STEPS):
        want = oracle.step(grads[k], COEFS[k], k + 1)
        mp = cc.fp(master) if master is not None else None
        if rule == "adamw":
            compact.prl_host_compact_adamw(N, lr, wd, betas[0], betas[1], 1e-8, k + 1, np.float32(COEFS[k]), cc.fp(grads[k]), vp(p), mp, vp(m), vp(v),
                                           cc.MODES.index(mode), int(state_bf16), elem_offset, ordinal, seed)
        else:
            compact.prl_host_compact_lion(N, lr, wd, betas[0], betas[1], k + 1, np.float32(COEFS[k]), cc.fp(grads[k]), vp(p), mp, vp(m),
                                          cc.MODES.index(mode), int(state_bf16), elem_offset, ordinal, seed)
        got = {"param": p, "exp_avg": m, "master": master, "exp_avg_sq": v}
        for name, st in want.items():
            a, b = got[name], st.out
            assert a.dtype == b.dtype
            same = a.view(np.uint32 if a.dtype == np.float32 else np.uint16) == b.view(np.uint32 if b.dtype == np.float32 else np.uint16)
            assert same.all(), f"step {k + 1} {name}: entry {int(np.argmin(same))} differs"
            assert same[[3, 4, 5, 7, 8, N - 1]].all()  # (across the groups of 4 and of 8)
    if state_bf16 or mode == "stochastic":
        rounded_both_ways = {name: (cc.bits32(st.pre) & 0xFFFF != 0).mean() for name, st in want.items() if st.addend is not None}
        assert all(share > 0.9 for share in rounded_both_ways.values()), "the inputs exercise the rounding"


def test_parameter_drift_is_unbiased_and_nearest_is_stuck(libs):
    """N bf16 parameters at 1.0, gradient 1, lr 1e-5, 200 AdamW steps: an update of 1e-5 is 1/390 of the bf16 spacing below 1.0.
    Compact state + stochastic parameters follow the fp64 witness in the mean; round-to-nearest never leaves 1.0."""
    optmath, _ = libs
    e = cc.DRIFT
    one = np.full(e["n"], 0x3F80, np.uint16)
    g = np.full(e["n"], e["g"], np.float32)
    sr_run = cc.CompactOracle(optmath, "adamw", "stochastic", True, one, lr=e["lr"], wd=0.0, betas=(0.9, 0.999), seed=0)
    nearest = cc.CompactOracle(optmath, "adamw", "nearest", False, one, lr=e["lr"], wd=0.0, betas=(0.9, 0.999))
    for t in range(1, e["steps"] + 1):
        sr_run.step(g, 1.0, t)
        nearest.step(g, 1.0, t)
    assert np.all(nearest.p == 0x3F80), "master_weights=False with round-to-nearest: every update is rounded away"
    cc.assert_within_standard_errors("oracle parameter drift", cc.widen(sr_run.p), cc.adamw_witness_fp64(e["p0"], e["g"], e["lr"], e["steps"]))


def test_second_moment_decay_is_unbiased_and_nearest_is_stuck(libs):
    """Zero gradient, exp_avg_sq = 1.0, 200 steps of v <- 0.999 v: 0.1 % per step is below half a bf16 ulp (0.2 - 0.4 %)."""
    optmath, _ = libs
    e = cc.DECAY
    n = e["n"]
    run = cc.CompactOracle(optmath, "adamw", "stochastic", True, np.full(n, 0x3F80, np.uint16), v=np.full(n, 0x3F80, np.uint16), lr=1e-5, wd=0.0,
                           betas=(0.9, e["beta2"]), seed=0)
    stuck = np.full(n, 0x3F80, np.uint16)
    zero = np.zeros(n, np.float32)
    for t in range(1, e["steps"] + 1):
        run.step(zero, 1.0, t)
        stuck = cc.rne(cc.widen(stuck) * np.float32(e["beta2"]))
    assert np.all(stuck == 0x3F80), "a round-to-nearest bf16 second moment cannot decay"
    assert np.all(run.p == 0x3F80) and np.all(run.m == 0), "zero gradient: nothing else moves"
    cc.assert_within_standard_errors("oracle second-moment decay", cc.widen(run.v), e["beta2"] ** e["steps"])


def test_header_and_harness_are_clean_under_the_host_sanitizers(tmp_path):
    """A stand-alone program (its own main) over the header and the harness, built with AddressSanitizer and
    UndefinedBehaviorSanitizer and run on its own: host code only, nothing sanitized is loaded into this process."""
    exe = tmp_path / "optim_compact_sanitize"
    subprocess.check_call(["g++", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{cc.ROOT / 'include'}",
                           "-o", str(exe), str(cc.ROOT / "tests" / "harness" / "optim_compact_sanitize_main.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr[-3000:]
