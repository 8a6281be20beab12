"""The arithmetic of the fused body kernels (pipelinerl_amd/csrc/prl_body_math.h), compiled for the host with g++
-ffp-contract=off and summed in the kernels' own order (tests/harness/body_math_host.cpp), against the fp64 witnesses under the
bounds of tests/body_checks.py; the reference's own values re-measured; and the bounds against seeded mistakes.  This checks the
device MATH and the acceptance rule on a machine without a GPU; the kernels are covered by tests/test_gpu_body.py."""

import ctypes
import subprocess
from pathlib import Path

import pytest
import torch

import body_checks as bc
from pipelinerl_amd._lib import BODY_GEOMETRY as GEOM

ROOT = Path(__file__).resolve().parent.parent
F = ctypes.POINTER(ctypes.c_float)
SPECIAL_COLS = (9, 896, 5120)     # the all-zero row and the 1e-20 row, scalar and vector widths
EDGE_NUMELS = (70, 2049)          # gate cycling through body_checks.GATE_EDGES


def fp(t):
    return ctypes.cast(t.data_ptr(), F)


@pytest.fixture(scope="module")
def bodymath(tmp_path_factory):
    out = tmp_path_factory.mktemp("harness") / "libbodymath.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", f"-I{ROOT / 'include'}", "-o", str(out),
                           str(ROOT / "tests" / "harness" / "body_math_host.cpp")])
    lib = ctypes.CDLL(str(out))
    lib.prl_host_rmsnorm_fwd.restype = None
    lib.prl_host_rmsnorm_fwd.argtypes = [ctypes.c_long, ctypes.c_long, ctypes.c_int, F, F, ctypes.c_float, F, F]
    lib.prl_host_rmsnorm_bwd.restype = None
    lib.prl_host_rmsnorm_bwd.argtypes = [ctypes.c_long, ctypes.c_long, ctypes.c_int] + [F] * 6
    lib.prl_host_swiglu_fwd.restype = None
    lib.prl_host_swiglu_fwd.argtypes = [ctypes.c_long] + [F] * 3
    lib.prl_host_swiglu_bwd.restype = None
    lib.prl_host_swiglu_bwd.argtypes = [ctypes.c_long] + [F] * 5
    return lib


def host_rmsnorm(lib, x, w, g, vec, eps=bc.EPS):
    x, w, g = x.contiguous(), w.contiguous(), g.contiguous()
    rows, cols = x.shape
    out, dx = torch.empty_like(x), torch.empty_like(x)
    rstd, dw = torch.empty(rows), torch.empty(cols)
    lib.prl_host_rmsnorm_fwd(rows, cols, vec, fp(x), fp(w), eps, fp(out), fp(rstd))
    lib.prl_host_rmsnorm_bwd(rows, cols, vec, fp(x), fp(w), fp(rstd), fp(g), fp(dx), fp(dw))
    return {"out": out, "rstd": rstd, "dx": dx, "dw": dw}


def host_swiglu(lib, gate, up, g):
    out, dg, du = torch.empty_like(gate), torch.empty_like(gate), torch.empty_like(gate)
    lib.prl_host_swiglu_fwd(gate.numel(), fp(gate), fp(up), fp(out))
    lib.prl_host_swiglu_bwd(gate.numel(), fp(gate), fp(up), fp(g), fp(dg), fp(du))
    return {"out": out, "d_gate": dg, "d_up": du}


def rmsnorm_cases():
    """(label, x, w, g) of the family BODY_REF is taken over: every H of both vector widths x every R, and the special rows."""
    cols = sorted(set(bc.rmsnorm_cols(GEOM, True)) | set(bc.rmsnorm_cols(GEOM, False)))
    for h in cols:
        for r in bc.rmsnorm_rows(GEOM):
            yield (f"[{r}, {h}]",) + bc.rmsnorm_inputs(r, h)
    for h in SPECIAL_COLS:
        yield (f"[4, {h}] zero row, 1e-20 row",) + bc.rmsnorm_inputs(4, h, special=True)


def swiglu_cases():
    for n in bc.swiglu_numels(GEOM) + [bc.SWIGLU_MODEL_SHAPE[0] * bc.SWIGLU_MODEL_SHAPE[1]]:
        yield (f"numel {n}",) + bc.swiglu_inputs(n)
    for n in EDGE_NUMELS:
        yield (f"numel {n} gate edges",) + bc.swiglu_inputs(n, edges=True)


def test_geometry_of_the_header_is_what_the_package_exports(bodymath):
    buf = (ctypes.c_int * 8)()
    assert bodymath.prl_host_body_geometry(buf) == 7
    names = ("block", "wave", "rows_per_block", "vec_bf16", "vec_f32", "band_rows", "swiglu_vec")
    assert dict(zip(names, list(buf)[:7])) == GEOM


def test_reference_stays_within_what_is_written():
    """BODY_REF is the reference's own worst value: re-measured here, it may not exceed what body_checks states, and the stated
    value is not padded (the measured one is at least half of it for every output)."""
    worst = {op: {k: 0.0 for k in v} for op, v in bc.BODY_REF.items()}
    for label, x, w, g in rmsnorm_cases():
        ref, wit = bc.reference_rmsnorm(x, w, g), bc.rmsnorm_witness(x, w, g)
        for k, v in ref.items():
            res = bc.measure(k, v, *wit[k])
            assert res.ok(bc.BODY_REF["rmsnorm"][k]), f"reference rmsnorm {label}: {res}"
            worst["rmsnorm"][k] = max(worst["rmsnorm"][k], res.err)
    for label, gate, up, g in swiglu_cases():
        ref, wit = bc.reference_swiglu(gate, up, g), bc.swiglu_witness(gate, up, g)
        for k, v in ref.items():
            res = bc.measure(k, v, *wit[k])
            assert res.ok(bc.BODY_REF["swiglu"][k]), f"reference swiglu {label}: {res}"
            worst["swiglu"][k] = max(worst["swiglu"][k], res.err)
    print("[body] reference, measured:", worst)
    for op, d in worst.items():
        for k, v in d.items():
            assert v >= 0.5 * bc.BODY_REF[op][k], (op, k, v, bc.BODY_REF[op][k])


@pytest.mark.parametrize("vec", [GEOM["vec_bf16"], GEOM["vec_f32"]])
def test_header_rmsnorm_within_the_bounds(bodymath, vec):
    worst = {}
    for label, x, w, g in rmsnorm_cases():
        errs = bc.check_outputs("rmsnorm", f"host V={vec} {label}", host_rmsnorm(bodymath, x, w, g, vec), bc.rmsnorm_witness(x, w, g), verbose=False)
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in errs.items()}
    print(f"[body] header rmsnorm V={vec}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def test_header_swiglu_within_the_bounds(bodymath):
    worst = {}
    for label, gate, up, g in swiglu_cases():
        errs = bc.check_outputs("swiglu", f"host {label}", host_swiglu(bodymath, gate, up, g), bc.swiglu_witness(gate, up, g), verbose=False)
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in errs.items()}
    print("[body] header swiglu: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def test_header_at_the_listed_points(bodymath):
    """Every gate of GATE_EDGES by itself, up = g = 1: finite, exactly 0 where the function is (gate = 0: out and d_up), and
    within the bounds; a row whose variance (1e-40) is far below eps has rstd = 1 / sqrt(eps) to fp32."""
    for z in bc.GATE_EDGES:
        gate, one = torch.tensor([z]), torch.ones(1)
        got = host_swiglu(bodymath, gate, one, one)
        assert all(torch.isfinite(v).all() for v in got.values()), (z, got)
        bc.check_outputs("swiglu", f"gate {z}", got, bc.swiglu_witness(gate, one, one), verbose=False)
        if z == 0.0:
            assert float(got["out"]) == 0.0 and float(got["d_up"]) == 0.0 and float(got["d_gate"]) == 0.5
    x = bc.bf16_exact(torch.randn(1, 896, generator=torch.Generator().manual_seed(1)) * 1e-20)
    got = host_rmsnorm(bodymath, x, torch.ones(896), torch.ones(1, 896), GEOM["vec_bf16"])
    assert abs(float(got["rstd"]) * bc.EPS ** 0.5 - 1.0) < 2.0 ** -22


@pytest.mark.parametrize("mistake", bc.RMSNORM_MISTAKES)
def test_bounds_flag_seeded_rmsnorm_mistakes(mistake):
    """The fp64 restatement is inside every bound on every case; with the mistake it is outside on at least one."""
    flagged = 0
    for label, x, w, g in rmsnorm_cases():
        wit = bc.rmsnorm_witness(x, w, g)
        bc.check_outputs("rmsnorm", f"restated {label}", bc.restated_rmsnorm(x, w, g, band_rows=GEOM["band_rows"]), wit, verbose=False)
        try:
            bc.check_outputs("rmsnorm", f"{mistake} {label}", bc.restated_rmsnorm(x, w, g, mistake=mistake, band_rows=GEOM["band_rows"]), wit, verbose=False)
        except AssertionError:
            flagged += 1
    assert flagged, f"the bounds accepted '{mistake}' on every case"
    print(f"[body] {mistake}: flagged on {flagged} cases")


@pytest.mark.parametrize("mistake", bc.SWIGLU_MISTAKES)
def test_bounds_flag_seeded_swiglu_mistakes(mistake):
    flagged = 0
    for label, gate, up, g in swiglu_cases():
        wit = bc.swiglu_witness(gate, up, g)
        bc.check_outputs("swiglu", f"restated {label}", bc.restated_swiglu(gate, up, g), wit, verbose=False)
        try:
            bc.check_outputs("swiglu", f"{mistake} {label}", bc.restated_swiglu(gate, up, g, mistake=mistake), wit, verbose=False)
        except AssertionError:
            flagged += 1
    assert flagged, f"the bounds accepted '{mistake}' on every case"
