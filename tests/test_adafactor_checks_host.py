"""The Adafactor pieces the HIP kernels execute (pipelinerl_amd/csrc/prl_adafactor_math.h), compiled for the host with
g++ -ffp-contract=off, against transformers' Adafactor under the per-entry bound of tests/adafactor_checks.py; and the checker
itself against seeded mistakes.  This checks the device MATH and the acceptance rule on a machine without a GPU; the kernels are
covered by tests/test_gpu_adafactor.py.

r_ref, the fp32 library step's own worst ratio against the fp64 witness (printed by every check; measured on the CPU, torch 2.10,
transformers 5.15), on these shapes and seeds: <= 3.4e-7 on factored parameters, <= 1.5e-7 on unfactored ones, <= 2.4e-7 on the averages
(<= 5.3e-7 over the other seeds tried when the reference was chosen: tests/adafactor_checks.py)."""

import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

from adafactor_checks import HYPER, adafactor_steps, check_entries, check_step, clip_case_grads, log_uniform_grads, restated_step

ROOT = Path(__file__).resolve().parent.parent
F = ctypes.POINTER(ctypes.c_float)
D = ctypes.c_double
SHAPES = [(67, 129), (1000,), (2, 3, 65), (1, 300), (300, 1), (1, 1), (5,)]


def fp(a):
    return a.ctypes.data_as(F)


@pytest.fixture(scope="module")
def adamath(tmp_path_factory):
    out = tmp_path_factory.mktemp("harness") / "libadamath.so"
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", f"-I{ROOT / 'include'}", "-o", str(out),
                           str(ROOT / "tests" / "harness" / "adafactor_math_host.cpp")])
    lib = ctypes.CDLL(str(out))
    lib.prl_host_adafactor.restype = None
    lib.prl_host_adafactor.argtypes = [ctypes.c_long] * 3 + [ctypes.c_int] + [D] * 5 + [ctypes.c_long, ctypes.c_float] + [F] * 5
    return lib


def host_step(lib, rec, lr, wd):
    """One step of the harness from the witness's state before it (rounded to fp32)."""
    before, g = rec["before"], np.ascontiguousarray(rec["g"], dtype=np.float32)
    shape = g.shape
    p = np.ascontiguousarray(before["p"], dtype=np.float32).copy()
    factored = len(shape) >= 2
    if factored:
        R, C = shape[-2:]
        B = int(np.prod(shape[:-2]))
        row = np.ascontiguousarray(before.get("exp_avg_sq_row", np.zeros(shape[:-1])), dtype=np.float32).copy()
        col = np.ascontiguousarray(before.get("exp_avg_sq_col", np.zeros(shape[:-2] + shape[-1:])), dtype=np.float32).copy()
        v = np.zeros(1, np.float32)
    else:
        B, R, C = 1, 1, shape[0]
        row = col = np.zeros(1, np.float32)
        v = np.ascontiguousarray(before.get("exp_avg_sq", np.zeros(shape)), dtype=np.float32).copy()
    lib.prl_host_adafactor(B, R, C, int(factored), lr, wd, HYPER["eps1"], HYPER["clip_threshold"], HYPER["decay_rate"], rec["step"],
                           np.float32(rec["coef"]), fp(g), fp(p), fp(row), fp(col), fp(v))
    return {"p": p, "exp_avg_sq_row": row, "exp_avg_sq_col": col} if factored else {"p": p, "exp_avg_sq": v}


def _inputs(shape, seed, steps=3):
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    p0 = rng.normal(0.0, 0.05, n).astype(np.float32).reshape(shape)
    grads = [g.reshape(shape) for g in log_uniform_grads(rng, n, steps)]
    for g in grads:
        g.flat[:: 7] = 0.0  # exact zeros: only eps1 keeps their squares away from 0
    return p0, grads


@pytest.mark.parametrize("wd", [0.01, 0.0])
@pytest.mark.parametrize("shape", SHAPES)
def test_header_reproduces_the_witness(adamath, shape, wd):
    lr, coefs = 1e-3, [1.0, 0.37, 0.0123]
    p0, grads = _inputs(shape, len(shape) * 1000 + shape[-1])
    worst = {}
    for rec in adafactor_steps(p0, grads, coefs, lr, wd):
        r = check_step(f"host adafactor {shape} wd={wd} step {rec['step']}", host_step(adamath, rec, lr, wd), rec)
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in r.items()}
    print(f"[adafactor] {shape} wd={wd}: r_ref = " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


@pytest.mark.parametrize("shape", [(67, 129), (1000,), (2, 3, 65)])
def test_float64_restatement_is_the_witness(shape):
    p0, grads = _inputs(shape, 5)
    for rec in adafactor_steps(p0, grads, [1.0, 0.37, 1.0], 1e-3, 0.01):
        got = restated_step(rec["before"], rec["g"], rec["coef"], rec["step"], 1e-3, 0.01, dtype=np.float64)
        for k, wit in rec["wit"].items():
            assert np.allclose(got[k], wit, rtol=1e-12, atol=0), (shape, rec["step"], k)
        # and in float32 it agrees with the library's state tensors under the bound (it is not the reference: see adafactor_checks)
        check_step(f"restated fp32 {shape} step {rec['step']}", restated_step(rec["before"], rec["g"], rec["coef"], rec["step"], 1e-3, 0.01), rec)


# ("eps1_dropped" shows on entries with a zero gradient of an unfactored parameter only - a mean hides it: its own test below)
MISTAKES = ["mean_over_wrong_axis", "beta2t_from_previous_step", "row_factor_not_normalised", "update_clip_omitted",
            "rms_per_matrix", "decay_after_update", "coef_after_square"]


@pytest.mark.parametrize("mistake", MISTAKES)
def test_checker_flags_seeded_mistakes(mistake):
    """lr and wd are large enough for the decay's place to matter; the matrices are square so that the wrong axis has the right
    shape; the gradients grow 10 x per step, differently per matrix of the batch, so that the update clip acts (rms > 1)."""
    rng = np.random.default_rng(9)
    shape, lr, wd = (3, 48, 48), 1e-2, 0.1
    p0 = rng.normal(0.0, 0.05, shape).astype(np.float32)
    grads = clip_case_grads("above", rng, shape)
    for g in grads[1:]:
        g[1] *= 0.05  # matrix 1 of the batch: rms(u) of its own differs from the parameter's
    for g in grads:
        g.flat[:: 7] = 0.0
    flagged = False
    for rec in adafactor_steps(p0, grads, [0.5, 0.37, 0.9], lr, wd)[1:]:  # steps 2 and 3 (step - 1 = 0 has no power)
        assert rec["ratio"] > 1.001
        check_step(f"unseeded step {rec['step']}", restated_step(rec["before"], rec["g"], rec["coef"], rec["step"], lr, wd), rec)
        try:
            check_step(f"{mistake} step {rec['step']}", restated_step(rec["before"], rec["g"], rec["coef"], rec["step"], lr, wd, mistake=mistake), rec)
        except AssertionError:
            flagged = True
    assert flagged, f"the checker accepted '{mistake}'"


def test_checker_flags_eps1_dropped_on_an_unfactored_parameter():
    p0, grads = _inputs((1000,), 3)
    rec = adafactor_steps(p0, grads, [1.0], 1e-3, 0.0)[0]
    with pytest.raises(AssertionError):
        check_step("eps1 dropped, 1-D", restated_step(rec["before"], rec["g"], 1.0, 1, 1e-3, 0.0, mistake="eps1_dropped"), rec)


@pytest.mark.parametrize("shape", [(67, 129), (1000,)])
@pytest.mark.parametrize("kind", ["below", "above"])
def test_update_clip_cases_are_away_from_one(kind, shape):
    """The gradients of the GPU test's two update-clip cases: the witness's rms / clip_threshold is >= 1e-3 away from 1 on steps 2
    and 3; on step 1 it is 1 up to eps1 for an unfactored parameter and near 1 for a factored one (the rank-1 estimate of g^2)."""
    rng = np.random.default_rng(77)
    p0 = rng.normal(0.0, 0.05, shape).astype(np.float32)
    recs = adafactor_steps(p0, clip_case_grads(kind, rng, shape), [1.0] * 3, 1e-3, 0.0)
    print(f"[adafactor] clip case {kind} {shape}: rms / clip = {[round(r['ratio'], 6) for r in recs]}")
    assert abs(recs[0]["ratio"] - 1.0) < (0.5 if len(shape) > 1 else 1e-3)
    for rec in recs[1:]:
        assert (rec["ratio"] < 1.0 - 1e-3) if kind == "below" else (rec["ratio"] > 1.0 + 1e-3)
