"""The per-element rule of the fp32 gradient fold (`prl_grad_accum_first` / `prl_grad_accum_add`, pipelinerl_amd/csrc/prl_optim_math.h),
compiled for the host with g++ -ffp-contract=off and compared with torch on the CPU: `g.float()` on the overwriting fold and
`acc + g.float()` afterwards, bit for bit (a NaN must be a NaN; its payload is not compared).  The kernel is covered by
tests/test_gpu_grad_accum.py."""

import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
F = ctypes.POINTER(ctypes.c_float)
H = ctypes.POINTER(ctypes.c_uint16)
N = 200_003


@pytest.fixture(scope="module")
def accmath(tmp_path_factory):
    out = tmp_path_factory.mktemp("harness") / "libgradaccum.so"
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", f"-I{ROOT / 'include'}", "-o", str(out),
                           str(ROOT / "tests" / "harness" / "grad_accum_host.cpp")])
    lib = ctypes.CDLL(str(out))
    lib.prl_host_grad_accum_bf16.restype = None
    lib.prl_host_grad_accum_bf16.argtypes = [ctypes.c_long, H, F, ctypes.c_int]
    lib.prl_host_grad_accum_f32.restype = None
    lib.prl_host_grad_accum_f32.argtypes = [ctypes.c_long, F, F, ctypes.c_int]
    return lib


SPECIAL = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -3e-39, 1.1754944e-38, np.inf, -np.inf, np.nan, 3.3895314e38, -3.3895314e38, 1.0, -1.0, 256.0],
                   dtype=np.float32)
# bf16 bit patterns: +-0, smallest / largest subnormals, smallest normal, +-inf, two NaNs, largest finite, 1.0, 2^-133 (a subnormal)
SPECIAL_BF16 = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x007F, 0x807F, 0x0080, 0x7F80, 0xFF80, 0x7FC0, 0xFFC1, 0x7F7F, 0xFF7F, 0x3F80, 0x0040], dtype=np.uint16)


def log_uniform(rng, n, lo=-44.0, hi=38.0):
    """Magnitudes 10^U(lo, hi) with random signs: from fp32 subnormals to close to overflow."""
    return (np.where(rng.random(n) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(lo, hi, n)).astype(np.float32)


def inputs(rng, bf16):
    """(acc, g): random log-uniform pairs - partly of like magnitude, so that the add rounds - and EVERY special paired with every special."""
    acc = log_uniform(rng, N)
    g = log_uniform(rng, N)
    near = rng.random(N) < 0.5
    g[near] = (acc[near] * rng.uniform(-2.0, 2.0, near.sum())).astype(np.float32)
    if bf16:
        gs = SPECIAL_BF16
        g_bits = torch.from_numpy(g).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    else:
        gs = SPECIAL
        g_bits = g
    a_sp = np.repeat(SPECIAL, gs.size)
    g_sp = np.tile(gs, SPECIAL.size)
    return np.concatenate([acc, a_sp]), np.ascontiguousarray(np.concatenate([g_bits, g_sp]))


def same_bits(got, want):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "a NaN where torch has none, or the other way round"
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    return int(nan.sum())


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "f32"])
def test_fold_is_torchs_fp32_add_bit_for_bit(accmath, bf16):
    rng = np.random.default_rng(7 + bf16)
    acc0, g = inputs(rng, bf16)
    n = acc0.size
    if bf16:
        g_t = torch.from_numpy(g.view(np.int16)).view(torch.bfloat16)
        call = lambda a, ow: accmath.prl_host_grad_accum_bf16(n, g.ctypes.data_as(H), a.ctypes.data_as(F), ow)
    else:
        g_t = torch.from_numpy(g)
        call = lambda a, ow: accmath.prl_host_grad_accum_f32(n, g.ctypes.data_as(F), a.ctypes.data_as(F), ow)
    sub = np.abs(g_t.float().numpy())
    assert ((sub > 0) & (sub < 1.1754944e-38)).sum() > 100, "the inputs reach the subnormals"
    add = acc0.copy()
    call(add, 0)
    nans = same_bits(add, (torch.from_numpy(acc0) + g_t.float()).numpy())
    assert nans >= 2 * SPECIAL.size  # NaN + x, x + NaN, inf - inf
    first = acc0.copy()
    first[:] = np.nan  # the overwriting fold does not read the accumulator
    call(first, 1)
    same_bits(first, g_t.float().numpy())
    if not bf16:
        keep = ~np.isnan(g)
        assert np.array_equal(first.view(np.uint32)[keep], g.view(np.uint32)[keep])


def test_a_bf16_running_sum_stalls_where_the_fp32_fold_does_not(accmath):
    """The reason for the accumulator, in the header's own arithmetic: 512 folds of bf16 1.0 give 512.0; the same sum kept in bf16 stops at 256."""
    n = 64
    g = np.full(n, 0x3F80, np.uint16)
    acc = np.full(n, np.nan, np.float32)
    for k in range(512):
        accmath.prl_host_grad_accum_bf16(n, g.ctypes.data_as(H), acc.ctypes.data_as(F), int(k == 0))
    assert np.all(acc == 512.0)
    s = torch.ones(n, dtype=torch.bfloat16)
    for _ in range(511):
        s += torch.ones(n, dtype=torch.bfloat16)
    assert torch.all(s == 256.0)
