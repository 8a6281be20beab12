"""The slice-form attention kernels on the GPU, in one process: the P slices of a row run one after the other and their fp32
dK / dV partials are folded in slice order.  Out, lse, dq and the folded dk, dv against the fp64 witness of the whole row under
the bounds of tests/attention_sp_checks.py; slices at a multiple of 64 and the single slice P = 1 against the square op bit for
bit; two runs; key blocks before the sweep start and rows past the slice never read, partial rows past the slice exact zeros;
strided views against copied layouts; the workspace's contents."""

import ctypes

import pytest
import torch

import attention_checks as ac
import attention_sp_checks as sp
from pipelinerl_amd import _lib
from pipelinerl_amd import fused_attention as fa
from pipelinerl_amd.fused_attention import BK, fold_parts, varlen_attention, varlen_attention_slice

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in sp.CASES}


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b)), f"{what} differs"


def square(q, k, v, g, ss, se, scale, device) -> dict:
    qd, kd, vd = (t.to(device=device, dtype=torch.bfloat16).requires_grad_(True) for t in (q, k, v))
    out, lse = varlen_attention(qd, kd, vd, ss.to(device), se.to(device), scale, return_lse=True)
    out.backward(g.to(device=device, dtype=torch.bfloat16))
    torch.cuda.synchronize(device)
    return {"out": out.detach().cpu(), "lse": lse.cpu(), "dq": qd.grad.cpu(), "dk": kd.grad.cpu(), "dv": vd.grad.cpu()}


def one_slice(q, k_all, v_all, g, ss, se, scale, q_off, nq, device) -> dict:
    """Forward and backward of the slice [q_off, q_off + nq): q / g are those rows of the whole-row tensors."""
    qd = q[q_off:q_off + nq].to(device=device, dtype=torch.bfloat16).requires_grad_(True)
    kd, vd = (t.to(device=device, dtype=torch.bfloat16) for t in (k_all, v_all))
    parts = []
    out, lse = varlen_attention_slice(qd, kd, vd, ss.to(device), se.to(device), q_off, scale, return_lse=True, kv_grad_parts=parts)
    out.backward(g[q_off:q_off + nq].to(device=device, dtype=torch.bfloat16))
    torch.cuda.synchronize(device)
    assert out.dtype == torch.bfloat16 and out.shape == (nq,) + tuple(q.shape[1:]) and lse.dtype == torch.float32 and lse.shape == (q.shape[1], nq)
    (dkp, dvp), = parts
    assert dkp.dtype == dvp.dtype == torch.float32 and dkp.shape == dvp.shape == tuple(k_all.shape)
    return {"out": out.detach().cpu(), "lse": lse.cpu(), "dq": qd.grad.cpu(), "dk_part": dkp, "dv_part": dvp}


def serial(q, k, v, g, ss, se, scale, p, device) -> dict:
    """The five results of the whole row from P slices run one after the other, the partials folded in slice order on the GPU."""
    length = q.shape[0] // p
    runs = [one_slice(q, k, v, g, ss, se, scale, r * length, length, device) for r in range(p)]
    return {
        "out": torch.cat([r["out"] for r in runs]), "lse": torch.cat([r["lse"] for r in runs], dim=1), "dq": torch.cat([r["dq"] for r in runs]),
        "dk": fold_parts(torch.stack([r["dk_part"] for r in runs])).cpu(), "dv": fold_parts(torch.stack([r["dv_part"] for r in runs])).cpu(),
        "runs": runs,
    }


@pytest.mark.parametrize("d", sp.HEAD_SIZES)
@pytest.mark.parametrize("heads", sp.HEADS, ids=lambda h: f"{h[0]}q{h[1]}kv")
@pytest.mark.parametrize("name", list(CASES))
def test_slices_against_the_witness_and_the_square_op(libprl, cuda_device, name, heads, d):
    case = CASES[name]
    q, k, v, g, scale, ss, se = sp.problem(case, heads[0], heads[1], d)
    got = serial(q, k, v, g, ss, se, scale, case.p, cuda_device)
    runs = got.pop("runs")
    sp.check_outputs(name, f"{name} {heads[0]}/{heads[1]} heads d {d}, {case.p} slices", got, ac.witness(q, k, v, g, ss, scale))
    # a slice at a multiple of 64 walks the square kernel's tiles in its order: the same bits
    whole = square(q, k, v, g, ss, se, scale, cuda_device)
    length, aligned = case.slice_len, 0
    for r, run in enumerate(runs):
        rows = slice(r * length, (r + 1) * length)
        if (r * length) % BK == 0:
            aligned += 1
            same(run["out"], whole["out"][rows], f"{name} slice {r}: out")
            same(run["lse"], whole["lse"][:, rows].contiguous(), f"{name} slice {r}: lse")
            same(run["dq"], whole["dq"][rows], f"{name} slice {r}: dq")
        # no local query sees a key past the slice: those rows of the partials are exact zeros (sign included)
        for part in (run["dk_part"], run["dv_part"]):
            assert not part[(r + 1) * length:].view(torch.int32).any(), f"{name} slice {r}: partial rows past the slice"
    assert aligned >= (2 if name != "sp_unaligned" else 1)


@pytest.mark.parametrize("d", sp.HEAD_SIZES)
@pytest.mark.parametrize("name", ["sp_unaligned", "sp_four", "sp_long"])
def test_one_slice_is_the_square_op_bit_for_bit(libprl, cuda_device, name, d):
    """P = 1 (q_off = 0, nq = nk): out, lse, dq are the square op's, and the one-part fold is its dk, dv."""
    case = CASES[name]
    q, k, v, g, scale, ss, se = sp.problem(case, 4, 2, d)
    got = serial(q, k, v, g, ss, se, scale, 1, cuda_device)
    whole = square(q, k, v, g, ss, se, scale, cuda_device)
    for out in ac.OUTPUTS:
        same(got[out], whole[out], f"{name} d {d}, one slice: {out}")


def test_two_runs_give_the_same_bits(libprl, cuda_device):
    for name, heads, d in (("sp_unaligned", (7, 1), 128), ("sp_four", (4, 2), 64), ("sp_long", (4, 2), 128)):
        case = CASES[name]
        q, k, v, g, scale, ss, se = sp.problem(case, heads[0], heads[1], d)
        a = serial(q, k, v, g, ss, se, scale, case.p, cuda_device)
        b = serial(q, k, v, g, ss, se, scale, case.p, cuda_device)
        for out in ac.OUTPUTS:
            same(a[out], b[out], f"{name}, second run: {out}")
        for ra, rb in zip(a["runs"], b["runs"]):
            same(ra["dk_part"].cpu(), rb["dk_part"].cpu(), f"{name}, second run: dk partial")
            same(ra["dv_part"].cpu(), rb["dv_part"].cpu(), f"{name}, second run: dv partial")


@pytest.mark.parametrize("d", sp.HEAD_SIZES)
def test_keys_outside_the_sweep_are_never_read(libprl, cuda_device, d):
    """The third slice of "sp_four" (queries 192 .. 287; its first query's sequence starts at 97): NaN in k_all / v_all of the key
    block [0, 64) - wholly before the sweep start - and of the rows from 288 on changes no bit; everything stays finite."""
    case = CASES["sp_four"]
    q, k, v, g, scale, ss, se = sp.problem(case, 4, 2, d)
    q_off, nq = 2 * case.slice_len, case.slice_len
    first_block = int(ss[q_off]) // BK * BK
    assert first_block == BK and q_off + nq < case.n
    base = one_slice(q, k, v, g, ss, se, scale, q_off, nq, cuda_device)
    kp, vp = k.clone(), v.clone()
    for t in (kp, vp):
        t[:first_block] = float("nan")
        t[q_off + nq:] = float("nan")
    got = one_slice(q, kp, vp, g, ss, se, scale, q_off, nq, cuda_device)
    for name in ("out", "lse", "dq", "dk_part", "dv_part"):
        assert torch.isfinite(got[name]).all(), name
        same(got[name].cpu(), base[name].cpu(), f"poisoned keys outside the sweep: {name}")
    for part in (got["dk_part"], got["dv_part"]):
        assert not part[q_off + nq:].view(torch.int32).any() and not part[:first_block].view(torch.int32).any()
        assert part[first_block:q_off + nq].any()


def test_strided_views_and_copied_layouts_give_the_same_bits(libprl, cuda_device):
    """q as a view of a fused [nq, Hq + 2 Hkv, D] projection output and k_all / v_all as views of one gathered [nk, 2 Hkv, D] buffer
    (no copy) against separate contiguous tensors, and against a layout whose D stride is 2 (copied once)."""
    case, (hq, hkv), d = CASES["sp_unaligned"], (4, 2), 64
    q, k, v, g, scale, ss, se = sp.problem(case, hq, hkv, d)
    q_off = nq = case.slice_len
    ssd, sed = ss.to(cuda_device), se.to(cuda_device)
    fused = torch.cat([q[q_off:], k[q_off:], v[q_off:]], dim=1).to(device=cuda_device, dtype=torch.bfloat16)
    gathered = torch.cat([k, v], dim=1).to(device=cuda_device, dtype=torch.bfloat16)
    gd = g[q_off:].to(device=cuda_device, dtype=torch.bfloat16)

    def go(make):
        leaf = fused.clone().requires_grad_(True)
        parts = []
        qq, kk, vv = make(leaf, gathered)
        out, lse = varlen_attention_slice(qq, kk, vv, ssd, sed, q_off, scale, return_lse=True, kv_grad_parts=parts)
        out.backward(gd)
        return {"out": out.detach(), "lse": lse, "dq": leaf.grad[:, :hq].contiguous(), "dk_part": parts[0][0], "dv_part": parts[0][1]}

    views = go(lambda f, kv: (f[:, :hq], kv[:, :hkv], kv[:, hkv:]))
    assert not gathered[:, hkv:].is_contiguous() and fa._rows_ok(gathered[:, hkv:]) and fa._rows_ok(fused[:, :hq])
    dense = go(lambda f, kv: (f[:, :hq].contiguous(), kv[:, :hkv].contiguous(), kv[:, hkv:].contiguous()))

    def every_other(x):
        wide = torch.stack([x, torch.zeros_like(x)], dim=-1).reshape(x.shape[0], x.shape[1], 2 * d)
        return wide[..., ::2]

    copied = go(lambda f, kv: (every_other(f[:, :hq]), every_other(kv[:, :hkv]), every_other(kv[:, hkv:])))
    assert not fa._rows_ok(every_other(gathered[:, :hkv]))
    for name in views:
        same(views[name], dense[name], f"views against contiguous tensors: {name}")
        same(views[name], copied[name], f"a layout that is copied once: {name}")
    ref = one_slice(q, k, v, g, ss, se, scale, q_off, nq, cuda_device)
    same(views["out"].cpu(), ref["out"], "views against the plain call: out")


def test_workspace_contents_do_not_matter(libprl, cuda_device):
    case, (hq, hkv), d = CASES["sp_unaligned"], (4, 2), 64
    q, k, v, g, scale, ss, se = sp.problem(case, hq, hkv, d)
    q_off = nq = case.slice_len
    nk = case.n
    base = one_slice(q, k, v, g, ss, se, scale, q_off, nq, cuda_device)
    qd, gd = (t[q_off:].to(device=cuda_device, dtype=torch.bfloat16).contiguous() for t in (q, g))
    kd, vd = (t.to(device=cuda_device, dtype=torch.bfloat16).contiguous() for t in (k, v))
    ssd, sed = ss.to(cuda_device), se.to(cuda_device)
    out, lse = base["out"].to(cuda_device), base["lse"].to(cuda_device)
    need = ctypes.c_size_t(0)
    _lib.check(libprl.prl_attn_slice_workspace_bytes(nq, hq, ctypes.byref(need)))
    ws = torch.full((need.value // 4 + 64,), float("nan"), dtype=torch.float32, device=cuda_device)
    dq = torch.empty_like(qd)
    dkp = torch.full((nk + 1, hkv, d), float("nan"), dtype=torch.float32, device=cuda_device)  # (a guard row behind each partial)
    dvp = torch.full((nk + 1, hkv, d), float("nan"), dtype=torch.float32, device=cuda_device)
    stream = torch.cuda.current_stream(cuda_device).cuda_stream
    _lib.check(libprl.prl_attn_slice_bwd(nq, nk, q_off, hq, hkv, d, qd.data_ptr(), hq * d, d, kd.data_ptr(), hkv * d, d, vd.data_ptr(), hkv * d, d, scale,
                                         ssd.data_ptr(), sed.data_ptr(), out.data_ptr(), lse.data_ptr(), gd.data_ptr(), dq.data_ptr(), dkp.data_ptr(),
                                         dvp.data_ptr(), ws.data_ptr(), need.value, stream))
    torch.cuda.synchronize(cuda_device)
    same(dq.cpu(), base["dq"], "NaN-filled workspace: dq")
    same(dkp[:nk].cpu(), base["dk_part"].cpu(), "NaN-filled workspace and NaN-filled partial buffers: dk partial")  # every element is written
    same(dvp[:nk].cpu(), base["dv_part"].cpu(), "NaN-filled workspace and NaN-filled partial buffers: dv partial")
    assert torch.isnan(ws[need.value // 4:]).all() and torch.isnan(dkp[nk]).all() and torch.isnan(dvp[nk]).all()  # nothing past the buffers


def test_fold_kernel_is_the_rank_order_sum(libprl, cuda_device):
    """The fold on the GPU against the same order in plain torch on the CPU, at lengths that take the 16-byte and the scalar form."""
    gen = torch.Generator().manual_seed(3)
    for p, n in ((1, 64), (2, 1000), (4, 4096 + 4), (3, 1001), (5, 3)):
        parts = torch.randn(p, n, generator=gen) * torch.logspace(-3, 3, p).view(p, 1)
        same(fold_parts(parts.to(cuda_device)).cpu(), fold_parts(parts), f"fold of {p} x {n}")
