"""The packed varlen attention kernels on the GPU: the segment kernel against `segments()` on the CPU bit for bit; forward and
backward against the fp64 witness under the per-entry bounds of tests/attention_checks.py (4 x the error of the flash
arithmetic on the CPU); isolation of packed sequences, two runs, the layouts of the upstream gradient, the scale as an argument,
skipped key blocks and the workspace bit for bit."""

import ctypes

import pytest
import torch

import attention_checks as ac
from pipelinerl_amd import _lib
from pipelinerl_amd import fused_attention as fa
from pipelinerl_amd.fused_attention import BK, BQ, segments, varlen_attention

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in ac.cases(BQ, BK)}


def run(q, k, v, g, ss, se, scale, device) -> dict:
    """The five results of one forward + backward on the GPU, as CPU tensors."""
    qd, kd, vd = (t.to(device=device, dtype=torch.bfloat16).requires_grad_(True) for t in (q, k, v))
    out, lse = varlen_attention(qd, kd, vd, ss.to(device), se.to(device), scale, return_lse=True)
    out.backward(g.to(device=device, dtype=torch.bfloat16))
    torch.cuda.synchronize(device)
    assert out.dtype == torch.bfloat16 and lse.dtype == torch.float32 and lse.shape == (q.shape[1], q.shape[0])
    return {"out": out.detach().cpu(), "lse": lse.cpu(), "dq": qd.grad.cpu(), "dk": kd.grad.cpu(), "dv": vd.grad.cpu()}


def same_bits(a: dict, b: dict, rows=None, what=""):
    for name in ac.OUTPUTS:
        x, y = a[name], b[name]
        if rows is not None:
            x, y = (x[:, rows], y[:, rows]) if name == "lse" else (x[rows], y[rows])
        assert torch.equal(x.view(torch.int16) if x.dtype == torch.bfloat16 else x.view(torch.int32),
                           y.view(torch.int16) if y.dtype == torch.bfloat16 else y.view(torch.int32)), f"{what}: {name} differs"


# ---- the segment kernel ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ac.segment_cases()))
def test_segment_kernel_equals_the_cpu_rule(libprl, cuda_device, name):
    pos, mask, shape = ac.segment_cases()[name]
    pos = None if pos is None else torch.tensor(pos)
    mask = None if mask is None else torch.tensor(mask)
    want = segments(pos, mask, shape)
    if pos is None and mask is None:
        return  # (no tensor names a device: this form is the CPU's)
    for mask_dtype in (torch.int64, torch.int32, torch.bool):
        got = segments(None if pos is None else pos.to(cuda_device), None if mask is None else mask.to(device=cuda_device, dtype=mask_dtype), shape)
        assert got[0].is_cuda and got[0].dtype == torch.int32
        assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1]), (name, mask_dtype)
        if mask is None:
            break


@pytest.mark.parametrize("t", [1, BK - 1, BK, BK + 1, 3 * BQ + 1, 2500])
def test_segment_kernel_sizes(libprl, cuda_device, t):
    pos, _, shape = ac.sized_segment_case(t)  # (2500: a thread of the kernel owns more than one token)
    pos = torch.tensor(pos)
    mask = (torch.arange(t) % 7 != 3).long().view(1, t)
    for p, m in ((pos, None), (pos, mask), (pos.expand(3, t).contiguous(), mask.expand(3, t).contiguous())):
        want = segments(p, m)
        got = segments(p.to(cuda_device), None if m is None else m.to(cuda_device))
        assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1]), (t, tuple(p.shape))


# ---- forward and backward against the witness ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", ac.HEAD_SIZES)
@pytest.mark.parametrize("heads", ac.HEADS, ids=lambda h: f"{h[0]}q{h[1]}kv")
@pytest.mark.parametrize("name", list(CASES))
def test_forward_and_backward_against_the_witness(libprl, cuda_device, name, heads, d):
    case = CASES[name]
    q, k, v, g, scale = ac.inputs(case, heads[0], heads[1], d)
    ss, se = ac.table_of(case.lengths)
    got = run(q, k, v, g, ss, se, scale, cuda_device)
    ac.check_outputs(name, f"{name} {heads[0]}/{heads[1]} heads d {d}", got, ac.witness(q, k, v, g, ss, scale))


def test_b2_and_padded_tables_come_from_segments(cuda_device):
    """The tables of the "b2" and "padded" cases are what segments() makes of a [2, T] batch and of a left- / right-padded one."""
    b2 = CASES["b2"]
    t = b2.lengths[0]
    got = segments(torch.arange(t, device=cuda_device).repeat(2, 1))
    want = ac.table_of(b2.lengths)
    assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1])
    mask = torch.ones(2, 40, dtype=torch.long)
    mask[0, :5] = 0
    mask[1, 30:] = 0
    got = segments(attention_mask=mask.to(cuda_device))
    want = ac.table_of(CASES["padded"].lengths)
    assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1])


# ---- layouts -------------------------------------------------------------------------------------------------------------------------
def test_strided_view_and_copied_layout_give_the_same_bits(libprl, cuda_device):
    """q, k, v as views of one token-major [N, Hq + 2 Hkv, D] buffer (no copy), as separate contiguous tensors, and in a layout
    whose D stride is 2 (copied once); then through the registered function from [B, H, T, D] views of token-major memory and
    from head-major tensors of B = 2 (which no [N, H, D] view can express)."""
    case, (hq, hkv), d = CASES["b2"], (4, 2), 64
    q, k, v, g, scale = ac.inputs(case, hq, hkv, d)
    ss, se = (t.to(cuda_device) for t in ac.table_of(case.lengths))
    n = case.n
    fused = torch.cat([q, k, v], dim=1).to(device=cuda_device, dtype=torch.bfloat16)
    gd = g.to(device=cuda_device, dtype=torch.bfloat16)

    def go(make):
        leaf = fused.clone().requires_grad_(True)
        qq, kk, vv = make(leaf)
        out, lse = varlen_attention(qq, kk, vv, ss, se, scale, return_lse=True)
        out.backward(gd)
        gr = leaf.grad
        return {"out": out.detach().cpu(), "lse": lse.cpu(), "dq": gr[:, :hq].cpu(), "dk": gr[:, hq:hq + hkv].cpu(), "dv": gr[:, hq + hkv:].cpu()}

    views = go(lambda f: (f[:, :hq], f[:, hq:hq + hkv], f[:, hq + hkv:]))
    assert not fused[:, hq:hq + hkv].is_contiguous() and fa._rows_ok(fused[:, hq:hq + hkv])
    dense = go(lambda f: (f[:, :hq].contiguous(), f[:, hq:hq + hkv].contiguous(), f[:, hq + hkv:].contiguous()))
    same_bits(views, dense, what="views of a fused buffer against contiguous tensors")

    def every_other(x):  # the same values at a D stride of 2
        wide = torch.stack([x, torch.zeros_like(x)], dim=-1).reshape(x.shape[0], x.shape[1], 2 * d)
        return wide[..., ::2]

    assert not fa._rows_ok(every_other(fused[:, :hq]))
    copied = go(lambda f: tuple(every_other(x) for x in (f[:, :hq], f[:, hq:hq + hkv], f[:, hq + hkv:])))
    same_bits(views, copied, what="a layout that is copied once")
    ac.check_outputs("b2", "views of a fused buffer", views, ac.witness(q, k, v, g, ss.cpu(), scale))

    # the registered function: [B, H, T, D]
    t = case.lengths[0]
    pos = torch.arange(t, device=cuda_device).repeat(2, 1)
    token_major = [x.view(2, t, -1, d).transpose(1, 2) for x in (fused[:, :hq], fused[:, hq:hq + hkv], fused[:, hq + hkv:])]
    head_major = [x.contiguous() for x in token_major]
    assert token_major[0].transpose(1, 2).reshape(n, hq, d).data_ptr() == fused.data_ptr()  # flattened without a copy
    a, _ = fa.prl_varlen_attention_forward(None, *token_major, None, scaling=scale, position_ids=pos)
    b, _ = fa.prl_varlen_attention_forward(None, *head_major, None, scaling=scale, position_ids=pos)
    assert a.shape == (2, t, hq, d) and torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert torch.equal(a.reshape(n, hq, d).cpu().view(torch.int16), views["out"].view(torch.int16))


# ---- isolation, bit for bit ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edges", "b2", "mid"])  # boundaries one before / on / one after a block edge and inside a block; "mid": mask-free tiles beyond it
def test_other_sequences_do_not_reach_a_sequence(libprl, cuda_device, name):
    case, (hq, hkv), d = CASES[name], (4, 2), 64
    q, k, v, g, scale = ac.inputs(case, hq, hkv, d)
    ss, se = ac.table_of(case.lengths)
    base = run(q, k, v, g, ss, se, scale, cuda_device)
    fresh = ac.inputs(case, hq, hkv, d, seed=12345)
    at = 0
    for length in case.lengths:
        keep = slice(at, at + length)
        at += length
        if length == 1:
            continue
        mixed = [f.clone() for f in fresh[:4]]
        for m, orig in zip(mixed, (q, k, v, g)):
            m[keep] = orig[keep]
        got = run(*mixed, ss, se, scale, cuda_device)
        same_bits(base, got, rows=keep, what=f"{name}: sequence at {keep.start} with every other sequence replaced")
        assert not torch.equal(base["out"], got["out"])  # (the others did change)


def test_two_runs_give_the_same_bits(libprl, cuda_device):
    for name, heads, d in (("edges", (7, 1), 128), ("long", (4, 2), 64), ("mid_ramp", (4, 2), 128)):
        case = CASES[name]
        q, k, v, g, scale = ac.inputs(case, heads[0], heads[1], d)
        ss, se = ac.table_of(case.lengths)
        same_bits(run(q, k, v, g, ss, se, scale, cuda_device), run(q, k, v, g, ss, se, scale, cuda_device), what=f"{name}: second run")


def test_upstream_gradient_layouts_give_the_same_bits(libprl, cuda_device):
    """The upstream gradient as a contiguous tensor, as a transposed view of head-major memory, as a slice of a wider buffer (its
    data_ptr() is not the start of an allocation) and as the expanded stride-0 tensor of `out.sum().backward()`: the same values
    give the same dq, dk, dv bit for bit."""
    case, (hq, hkv), d = CASES["edges"], (4, 2), 64
    q, k, v, g, scale = ac.inputs(case, hq, hkv, d)
    ss, se = (t.to(cuda_device) for t in ac.table_of(case.lengths))
    n = case.n
    gd = g.to(device=cuda_device, dtype=torch.bfloat16)

    def go(upstream):
        qd, kd, vd = (t.to(device=cuda_device, dtype=torch.bfloat16).requires_grad_(True) for t in (q, k, v))
        out, lse = varlen_attention(qd, kd, vd, ss, se, scale, return_lse=True)
        upstream(out)
        torch.cuda.synchronize(cuda_device)
        return {"out": out.detach().cpu(), "lse": lse.cpu(), "dq": qd.grad.cpu(), "dk": kd.grad.cpu(), "dv": vd.grad.cpu()}

    base = go(lambda out: out.backward(gd))
    ac.check_outputs("edges", "contiguous upstream gradient", base, ac.witness(q, k, v, g, ss.cpu(), scale))

    head_major = gd.transpose(0, 1).contiguous()  # [Hq, N, D]
    view = head_major.transpose(0, 1)
    assert not view.is_contiguous() and torch.equal(view, gd)
    same_bits(base, go(lambda out: out.backward(view)), what="a transposed view as the upstream gradient")

    wide = torch.zeros(n + 3, hq, d + 8, dtype=torch.bfloat16, device=cuda_device)
    wide[3:, :, 8:] = gd
    piece = wide[3:, :, 8:]
    assert piece.data_ptr() != wide.data_ptr() and not piece.is_contiguous() and torch.equal(piece, gd)
    same_bits(base, go(lambda out: out.backward(piece)), what="a slice of a wider buffer as the upstream gradient")
    for shift in (8, 4):  # contiguous, 16 and 8 bytes into its allocation: read where it lies / copied once to 16-byte alignment
        shifted = torch.zeros(n * hq * d + shift, dtype=torch.bfloat16, device=cuda_device)[shift:].view(n, hq, d)
        shifted.copy_(gd)
        assert shifted.is_contiguous() and shifted.data_ptr() % 32 == 2 * shift
        same_bits(base, go(lambda out: out.backward(shifted)), what=f"a contiguous upstream gradient {2 * shift} bytes into an allocation")

    ones = go(lambda out: out.backward(torch.ones_like(out)))
    same_bits(ones, go(lambda out: out.sum().backward()), what="the expanded stride-0 gradient of out.sum()")
    assert not torch.equal(ones["dq"], base["dq"])


def test_scale_is_an_argument(libprl, cuda_device):
    """scale and 2 x scale with q halved (exact in bf16): the products scale q . k are the same numbers, so out, lse, dk and dv are
    the same bits and dq is exactly twice (tests/test_attention_checks_host.py shows the flash arithmetic does just that).  A
    kernel with the scale fixed in one of its uses breaks one of them."""
    case, (hq, hkv), d = CASES["b2"], (4, 2), 64
    q, k, v, g, scale = ac.inputs(case, hq, hkv, d)
    ss, se = ac.table_of(case.lengths)
    assert torch.equal(ac.bf16_exact(0.5 * q), 0.5 * q)
    a = run(q, k, v, g, ss, se, scale, cuda_device)
    b = run(0.5 * q, k, v, g, ss, se, 2.0 * scale, cuda_device)
    ac.check_outputs("b2", "scale as given", a, ac.witness(q, k, v, g, ss, scale))
    twice = dict(a, dq=(2.0 * a["dq"].float()).to(torch.bfloat16))  # (a doubling is exact in bf16)
    same_bits(twice, b, what="scale doubled and q halved")


def test_key_blocks_before_the_sequence_start_are_not_read(libprl, cuda_device):
    """inf and NaN in k and v of a key block that lies wholly before the other sequences' start change nothing in them: the
    block is skipped, not multiplied by zero."""
    lengths, (hq, hkv), d = (BK, BK, BK + 1), (4, 2), 64
    case = ac.Case("poison", lengths)
    q, k, v, g, scale = ac.inputs(case, hq, hkv, d)
    ss, se = ac.table_of(lengths)
    base = run(q, k, v, g, ss, se, scale, cuda_device)
    kp, vp = k.clone(), v.clone()
    kp[:BK:3], kp[1:BK:3], kp[2:BK:3] = float("inf"), float("nan"), float("-inf")
    vp[:BK:2], vp[1:BK:2] = float("nan"), float("inf")
    got = run(q, kp, vp, g, ss, se, scale, cuda_device)
    same_bits(base, got, rows=slice(BK, case.n), what="poisoned first key block")
    assert not torch.isfinite(got["out"][:BK]).all()  # (the poisoned sequence itself is not compared)


def test_workspace_contents_do_not_matter(libprl, cuda_device):
    case, (hq, hkv), d = CASES["edges"], (4, 2), 64
    q, k, v, g, scale = ac.inputs(case, hq, hkv, d)
    ss, se = (t.to(cuda_device) for t in ac.table_of(case.lengths))
    base = run(q, k, v, g, ss, se, scale, cuda_device)
    n = case.n
    qd, kd, vd, gd = (t.to(device=cuda_device, dtype=torch.bfloat16).contiguous() for t in (q, k, v, g))
    out, lse = base["out"].to(cuda_device), base["lse"].to(cuda_device)
    need = ctypes.c_size_t(0)
    _lib.check(libprl.prl_attn_workspace_bytes(n, hq, ctypes.byref(need)))
    ws = torch.full((need.value // 4 + 64,), float("nan"), dtype=torch.float32, device=cuda_device)
    dq, dk, dv = torch.empty_like(qd), torch.empty_like(kd), torch.empty_like(vd)
    stream = torch.cuda.current_stream(cuda_device).cuda_stream
    _lib.check(libprl.prl_attn_varlen_bwd(n, hq, hkv, d, qd.data_ptr(), hq * d, d, kd.data_ptr(), hkv * d, d, vd.data_ptr(), hkv * d, d, scale,
                                          ss.data_ptr(), se.data_ptr(), out.data_ptr(), lse.data_ptr(), gd.data_ptr(), dq.data_ptr(), dk.data_ptr(),
                                          dv.data_ptr(), ws.data_ptr(), need.value, stream))
    torch.cuda.synchronize(cuda_device)
    same_bits(base, {"out": base["out"], "lse": base["lse"], "dq": dq.cpu(), "dk": dk.cpu(), "dv": dv.cpu()}, what="NaN-filled workspace")
    assert torch.isnan(ws[need.value // 4:]).all()  # nothing was written past the workspace


def test_offsets_past_2_to_the_31(libprl, cuda_device):
    """N x D past 2^31 elements (one head, D = 64, sequences of 48 tokens): the last sequences against the witness of their own
    tokens - an offset computed in 32 bits would read and write somewhere else."""
    d, length = 64, 48
    count = (1 << 31) // (d * length) + 3
    n = count * length
    assert n * d > (1 << 31)
    gen = torch.Generator(device=cuda_device).manual_seed(7)
    q, k, v, g = (torch.randn(n, 1, d, device=cuda_device, dtype=torch.bfloat16, generator=gen) for _ in range(4))
    q.requires_grad_(True), k.requires_grad_(True), v.requires_grad_(True)
    ss, se = segments(torch.arange(length, device=cuda_device).repeat(count).view(1, n))
    out, lse = varlen_attention(q, k, v, ss, se, d ** -0.5, return_lse=True)
    out.backward(g)
    torch.cuda.synchronize(cuda_device)
    tail = slice(n - 3 * length, n)
    assert int(ss[-1]) == n - length and int(se[-1]) == n
    got = {"out": out.detach()[tail].cpu(), "lse": lse[:, tail].cpu(), "dq": q.grad[tail].cpu(), "dk": k.grad[tail].cpu(), "dv": v.grad[tail].cpu()}
    local = ac.table_of((length,) * 3)[0]
    wit = ac.witness(q.detach()[tail].cpu(), k.detach()[tail].cpu(), v.detach()[tail].cpu(), g[tail].cpu(), local, d ** -0.5)
    ac.check_outputs("padded", "tail of 2^31 elements", got, wit)  # (the tightest row of the table: short sequences, unit scores)
