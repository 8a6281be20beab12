"""The fused RMSNorm / SwiGLU kernels (csrc/prl_body.hip) and `pipelinerl_amd.fused_body.rms_norm` / `swiglu` on the GPU.

Acceptance is per entry (tests/body_checks.py): fp64 witness, the size of each entry's own terms as the scale, bound = 4 x the
reference op sequence's own value of the metric.  Shapes sit on the kernels' edges, taken from the exported geometry."""

import ctypes

import pytest
import torch
import torch.utils.checkpoint

import body_checks as bc
from pipelinerl_amd import _lib
from pipelinerl_amd._lib import BODY_GEOMETRY as GEOM

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
PAIRS = [(BF16, BF16), (BF16, F32), (F32, BF16), (F32, F32)]  # (x, weight)
CODE = {F32: _lib.PRL_DTYPE_F32, BF16: _lib.PRL_DTYPE_BF16}
ALL_COLS = sorted(set(bc.rmsnorm_cols(GEOM, True)) | set(bc.rmsnorm_cols(GEOM, False)))
GUARD, CANARY = 64, 1536.0  # elements in front of and behind a guarded buffer; exact in bf16


def name(dt):
    return "bf16" if dt == BF16 else "f32"


def run_rmsnorm(x32, w32, g32, xdt, wdt, dev, shape=None):
    """forward + backward through the public function -> (outputs, roundings, the tensors autograd saved)"""
    from pipelinerl_amd.fused_body import rms_norm

    x = x32.to(xdt).to(dev)
    if shape is not None:
        x = x.reshape(shape)
    x.requires_grad_(True)
    w = w32.to(wdt).to(dev).requires_grad_(True)
    out = rms_norm(x, w, bc.EPS)
    assert out.dtype == torch.promote_types(xdt, wdt) and out.shape == x.shape
    saved = out.grad_fn.saved_tensors
    out.backward(g32.to(out.dtype).to(dev).reshape(out.shape))
    assert x.grad.dtype == xdt and w.grad.dtype == wdt
    got = {"out": out.detach(), "rstd": saved[2], "dx": x.grad, "dw": w.grad}
    rounding = {"out": bc.out_rounding(out.dtype), "rstd": 0.0, "dx": bc.out_rounding(xdt), "dw": bc.out_rounding(wdt)}
    return got, rounding, saved


def run_swiglu(gate32, up32, g32, dt, dev):
    from pipelinerl_amd.fused_body import swiglu

    gate = gate32.to(dt).to(dev).requires_grad_(True)
    up = up32.to(dt).to(dev).requires_grad_(True)
    out = swiglu(gate, up)
    assert out.dtype == dt and out.shape == gate.shape
    saved = out.grad_fn.saved_tensors
    out.backward(g32.to(dt).to(dev))
    return {"out": out.detach(), "d_gate": gate.grad, "d_up": up.grad}, {k: bc.out_rounding(dt) for k in ("out", "d_gate", "d_up")}, saved


# ---- RMSNorm ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", ALL_COLS)
def test_rmsnorm_per_entry(libprl, cuda_device, cols):
    """Every R of the family x all four dtype pairs at this H (the witness of a shape is shared by the pairs)."""
    for rows in bc.rmsnorm_rows(GEOM):
        x, w, g = bc.rmsnorm_inputs(rows, cols)
        wit = bc.rmsnorm_witness(x, w, g)
        for xdt, wdt in PAIRS:
            got, rounding, _ = run_rmsnorm(x, w, g, xdt, wdt, cuda_device)
            bc.check_outputs("rmsnorm", f"[{rows}, {cols}] x {name(xdt)} w {name(wdt)}", got, wit, rounding)


@pytest.mark.parametrize("cols", [9, 896, 5120])
def test_rmsnorm_zero_row_and_tiny_row(libprl, cuda_device, cols):
    """Row 1 is all zeros (out and its scale are exactly 0; dx = rstd g w), row 2 is 1e-20 x: its variance is far below eps."""
    x, w, g = bc.rmsnorm_inputs(4, cols, special=True)
    wit = bc.rmsnorm_witness(x, w, g)
    for xdt, wdt in PAIRS:
        got, rounding, _ = run_rmsnorm(x, w, g, xdt, wdt, cuda_device)
        bc.check_outputs("rmsnorm", f"[4, {cols}] special rows x {name(xdt)} w {name(wdt)}", got, wit, rounding)
        assert float(got["out"][1].abs().max()) == 0.0
        assert abs(float(got["rstd"][1]) * bc.EPS ** 0.5 - 1.0) < 2.0 ** -22 and abs(float(got["rstd"][2]) * bc.EPS ** 0.5 - 1.0) < 2.0 ** -22


@pytest.mark.parametrize("cols", [9, 896])
@pytest.mark.parametrize("xdt,wdt", [(BF16, BF16), (F32, F32)], ids=["bf16", "f32"])
def test_rmsnorm_leading_shape_and_non_contiguous_input(libprl, cuda_device, cols, xdt, wdt):
    """A [2, 3, H] input and a non-contiguous one give the bits of the flat contiguous call."""
    from pipelinerl_amd.fused_body import rms_norm

    x, w, g = bc.rmsnorm_inputs(6, cols)
    wit = bc.rmsnorm_witness(x, w, g)
    flat, rounding, _ = run_rmsnorm(x, w, g, xdt, wdt, cuda_device)
    bc.check_outputs("rmsnorm", f"[6, {cols}] {name(xdt)}", flat, wit, rounding)
    shaped, _, _ = run_rmsnorm(x, w, g, xdt, wdt, cuda_device, shape=(2, 3, cols))
    for k in flat:
        assert torch.equal(shaped[k].reshape(flat[k].shape), flat[k]), k
    # every second column of a [6, 2 H] buffer: strides (2 H, 2)
    wide = torch.zeros(6, 2 * cols, dtype=xdt, device=cuda_device)
    wide[:, ::2] = x.to(xdt).to(cuda_device)
    xs = wide[:, ::2].requires_grad_(True)
    assert not xs.is_contiguous()
    wd = w.to(wdt).to(cuda_device).requires_grad_(True)
    out = rms_norm(xs, wd, bc.EPS)
    gs = torch.zeros(6, 2 * cols, dtype=out.dtype, device=cuda_device)
    gs[:, ::2] = g.to(out.dtype).to(cuda_device)
    out.backward(gs[:, ::2])
    assert torch.equal(out.detach(), flat["out"]) and torch.equal(xs.grad, flat["dx"]) and torch.equal(wd.grad, flat["dw"])


class Guarded:
    """`values` inside a buffer of canaries, `off` elements off the allocation's 16-byte alignment."""

    def __init__(self, values, dtype, device, off=0):
        v = values.reshape(-1)
        self.n, self.lo = v.numel(), GUARD + off
        self.buf = torch.full((self.n + 2 * GUARD + off,), CANARY, dtype=dtype, device=device)
        self.view = self.buf[self.lo:self.lo + self.n]
        self.view.copy_(v.to(dtype))

    def ptr(self):
        return self.view.data_ptr()

    def intact(self):
        return bool((self.buf[:self.lo] == CANARY).all() and (self.buf[self.lo + self.n:] == CANARY).all())


def abi_rmsnorm(lib, dev, x32, w32, g32, xdt, wdt, off):
    """forward + backward through the C ABI on guarded buffers `off` elements off alignment -> dict of results"""
    rows, cols = x32.shape
    odt = torch.promote_types(xdt, wdt)
    x, w, g = Guarded(x32, xdt, dev, off), Guarded(w32, wdt, dev, off), Guarded(g32, odt, dev, off)
    out, dx = Guarded(torch.zeros(rows * cols), odt, dev, off), Guarded(torch.zeros(rows * cols), xdt, dev, off)
    rstd, dw = Guarded(torch.zeros(rows), F32, dev), Guarded(torch.zeros(cols), F32, dev)
    need = ctypes.c_size_t(0)
    _lib.check(lib.prl_rmsnorm_workspace_bytes(rows, cols, ctypes.byref(need)))
    assert need.value >= -(-rows // GEOM["band_rows"]) * cols * 4
    ws = Guarded(torch.zeros(need.value // 4), F32, dev)
    st = _lib.current_stream_ptr(dev)
    _lib.check(lib.prl_rmsnorm_fwd(rows, cols, x.ptr(), CODE[xdt], w.ptr(), CODE[wdt], bc.EPS, out.ptr(), rstd.ptr(), st))
    _lib.check(lib.prl_rmsnorm_bwd(rows, cols, x.ptr(), CODE[xdt], w.ptr(), CODE[wdt], rstd.ptr(), g.ptr(), dx.ptr(), dw.ptr(), ws.ptr(), need.value, st))
    torch.cuda.synchronize()
    for k, b in dict(x=x, w=w, g=g, out=out, dx=dx, rstd=rstd, dw=dw, ws=ws).items():
        assert b.intact(), f"a write outside {k} (off {off})"
    return {"out": out.view.clone().reshape(rows, cols), "rstd": rstd.view.clone(), "dx": dx.view.clone().reshape(rows, cols), "dw": dw.view.clone()}


@pytest.mark.parametrize("xdt,wdt", PAIRS, ids=[f"{name(a)}-{name(b)}" for a, b in PAIRS])
def test_rmsnorm_scalar_path_has_the_bits_of_the_vector_path(libprl, cuda_device, xdt, wdt):
    """Rows that do not start 16-byte aligned take the element-by-element path: same arithmetic order, so the same bits; and no
    kernel writes outside its arrays on either path (rows past one band, columns past one wave's width and a ragged tail)."""
    rows = GEOM["band_rows"] + 3
    for cols in (GEOM["wave"] * GEOM["vec_bf16"] + 8, 9):
        x, w, g = bc.rmsnorm_inputs(rows, cols)
        aligned = abi_rmsnorm(libprl, cuda_device, x, w, g, xdt, wdt, 0)
        shifted = abi_rmsnorm(libprl, cuda_device, x, w, g, xdt, wdt, 1)
        for k in aligned:
            assert torch.equal(aligned[k], shifted[k]), (k, cols)
        rounding = {"out": bc.out_rounding(aligned["out"].dtype), "dx": bc.out_rounding(xdt)}
        bc.check_outputs("rmsnorm", f"C ABI [{rows}, {cols}] x {name(xdt)} w {name(wdt)}", aligned, bc.rmsnorm_witness(x, w, g), rounding)


# ---- SwiGLU ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("numel", bc.swiglu_numels(GEOM) + [bc.SWIGLU_MODEL_SHAPE[0] * bc.SWIGLU_MODEL_SHAPE[1]])
def test_swiglu_per_entry(libprl, cuda_device, numel):
    gate, up, g = bc.swiglu_inputs(numel)
    wit = bc.swiglu_witness(gate, up, g)
    for dt in (BF16, F32):
        got, rounding, _ = run_swiglu(gate, up, g, dt, cuda_device)
        bc.check_outputs("swiglu", f"numel {numel} {name(dt)}", got, wit, rounding)


@pytest.mark.parametrize("numel", [70, 2049])
def test_swiglu_gate_edges(libprl, cuda_device, numel):
    """gate in {0, +-1e-30, +-20, +-88}: exactly 0 where the function is, finite and within the bounds everywhere."""
    gate, up, g = bc.swiglu_inputs(numel, edges=True)
    wit = bc.swiglu_witness(gate, up, g)
    for dt in (BF16, F32):
        got, rounding, _ = run_swiglu(gate, up, g, dt, cuda_device)
        bc.check_outputs("swiglu", f"numel {numel} gate edges {name(dt)}", got, wit, rounding)


@pytest.mark.parametrize("dt", [BF16, F32], ids=name)
def test_swiglu_unaligned_has_the_bits_of_the_vector_path(libprl, cuda_device, dt):
    numel = GEOM["block"] * GEOM["swiglu_vec"] + 13
    gate32, up32, g32 = bc.swiglu_inputs(numel)
    res = []
    for off in (0, 1):
        gate, up, g = (Guarded(t, dt, cuda_device, off) for t in (gate32, up32, g32))
        out, dg, du = (Guarded(torch.zeros(numel), dt, cuda_device, off) for _ in range(3))
        st = _lib.current_stream_ptr(cuda_device)
        _lib.check(libprl.prl_swiglu_fwd(numel, gate.ptr(), up.ptr(), CODE[dt], out.ptr(), st))
        _lib.check(libprl.prl_swiglu_bwd(numel, gate.ptr(), up.ptr(), g.ptr(), CODE[dt], dg.ptr(), du.ptr(), st))
        torch.cuda.synchronize()
        assert all(b.intact() for b in (gate, up, g, out, dg, du)), f"a write outside an array (off {off})"
        res.append({"out": out.view.clone(), "d_gate": dg.view.clone(), "d_up": du.view.clone()})
    for k in res[0]:
        assert torch.equal(res[0][k], res[1][k]), k
    bc.check_outputs("swiglu", f"C ABI numel {numel} {name(dt)}", res[0], bc.swiglu_witness(gate32, up32, g32), {k: bc.out_rounding(dt) for k in res[0]})


# ---- both ------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits(libprl, cuda_device):
    rows, cols = 2 * GEOM["band_rows"] + 1, 896
    x, w, g = bc.rmsnorm_inputs(rows, cols)
    for xdt, wdt in PAIRS:
        a, _, _ = run_rmsnorm(x, w, g, xdt, wdt, cuda_device)
        b, _, _ = run_rmsnorm(x, w, g, xdt, wdt, cuda_device)
        for k in a:
            assert torch.equal(a[k], b[k]), (k, xdt, wdt)
    gate, up, gg = bc.swiglu_inputs(GEOM["block"] * GEOM["swiglu_vec"] * 3 + 5)
    for dt in (BF16, F32):
        a, _, _ = run_swiglu(gate, up, gg, dt, cuda_device)
        b, _, _ = run_swiglu(gate, up, gg, dt, cuda_device)
        for k in a:
            assert torch.equal(a[k], b[k]), (k, dt)


def test_autograd_saves_what_it_says_and_nothing_under_no_grad(libprl, cuda_device):
    from pipelinerl_amd.fused_body import rms_norm, swiglu

    x, w, g = bc.rmsnorm_inputs(5, 72)
    _, _, saved = run_rmsnorm(x, w, g, BF16, BF16, cuda_device)
    assert [tuple(t.shape) for t in saved] == [(5, 72), (72,), (5,)] and saved[2].dtype == F32
    gate, up, gg = bc.swiglu_inputs(100)
    _, _, saved = run_swiglu(gate, up, gg, BF16, cuda_device)
    assert [tuple(t.shape) for t in saved] == [(100,), (100,)]
    xd = x.to(BF16).to(cuda_device).requires_grad_(True)
    wd = w.to(BF16).to(cuda_device).requires_grad_(True)
    with torch.no_grad():
        out = rms_norm(xd, wd, bc.EPS)
        act = swiglu(xd, xd)
    assert out.grad_fn is None and not out.requires_grad and act.grad_fn is None
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rms_norm(x, w, bc.EPS)
    with pytest.raises(TypeError):
        swiglu(xd.half(), xd.half())


@pytest.mark.parametrize("use_reentrant", [False, True])
def test_backward_under_checkpoint_has_the_same_bits(libprl, cuda_device, use_reentrant):
    from pipelinerl_amd.fused_body import rms_norm, swiglu

    x32, w32, g32 = bc.rmsnorm_inputs(GEOM["band_rows"] + 1, 136)

    def block(x, w):
        h = rms_norm(x, w, bc.EPS)
        return swiglu(h, h * 0.5)

    grads = []
    for ckpt in (False, True):
        x = x32.to(BF16).to(cuda_device).requires_grad_(True)
        w = w32.to(BF16).to(cuda_device).requires_grad_(True)
        out = torch.utils.checkpoint.checkpoint(block, x, w, use_reentrant=use_reentrant) if ckpt else block(x, w)
        out.backward(g32.to(BF16).to(cuda_device))
        grads.append((out.detach(), x.grad, w.grad))
    for a, b in zip(*grads):
        assert torch.equal(a, b)


def test_abi_argument_checks(libprl, cuda_device):
    """Bad arguments return PRL_EINVAL before any device work: the output buffers keep their canaries."""
    E = _lib.PRL_EINVAL
    buf = torch.full((4096,), CANARY, dtype=F32, device=cuda_device)
    p, st = buf.data_ptr(), _lib.current_stream_ptr(cuda_device)
    need = ctypes.c_size_t(0)
    lib = libprl
    assert lib.prl_rmsnorm_workspace_bytes(4, 8, None) == E
    assert lib.prl_rmsnorm_workspace_bytes(-1, 8, ctypes.byref(need)) == E
    assert lib.prl_rmsnorm_workspace_bytes(4, 0, ctypes.byref(need)) == E
    assert lib.prl_rmsnorm_workspace_bytes(GEOM["band_rows"] + 1, 8, ctypes.byref(need)) == 0 and need.value == 2 * 8 * 4
    fwd = lambda rows=4, cols=8, x=p, xd=0, w=p, wd=0, eps=1e-6, out=p, rstd=p: lib.prl_rmsnorm_fwd(rows, cols, x, xd, w, wd, eps, out, rstd, st)  # noqa: E731
    assert fwd(x=None) == E and fwd(w=None) == E and fwd(out=None) == E and fwd(rstd=None) == E
    assert b"null" in lib.prl_last_error()
    assert fwd(rows=-1) == E and fwd(cols=0) == E and fwd(cols=-8) == E and fwd(xd=2) == E and fwd(wd=-1) == E and fwd(eps=-1.0) == E
    assert fwd(rows=0, x=None, out=None, rstd=None) == 0
    bwd = lambda rows=4, cols=8, x=p, xd=0, w=p, wd=0, rstd=p, g=p, dx=p, dw=p, ws=p, nb=4096: lib.prl_rmsnorm_bwd(  # noqa: E731
        rows, cols, x, xd, w, wd, rstd, g, dx, dw, ws, nb, st)
    assert bwd(x=None) == E and bwd(rstd=None) == E and bwd(g=None) == E and bwd(w=None) == E and bwd(dx=None, dw=None) == E
    assert bwd(rows=-1) == E and bwd(cols=0) == E and bwd(xd=7) == E and bwd(wd=7) == E
    assert bwd(ws=None) == E and bwd(nb=8 * 4 - 1) == E and bwd(ws=p + 4) == E
    assert b"workspace" in lib.prl_last_error()
    assert bwd(rows=0, x=None, g=None, dx=None, dw=None) == E  # nothing is wanted
    sw = lambda n=8, a=p, b=p, dt=0, out=p: lib.prl_swiglu_fwd(n, a, b, dt, out, st)  # noqa: E731
    assert sw(a=None) == E and sw(b=None) == E and sw(out=None) == E and sw(n=-1) == E and sw(dt=5) == E
    assert sw(n=0, a=None, b=None, out=None) == 0
    sb = lambda n=8, a=p, b=p, g=p, dt=0, dg=p, du=p: lib.prl_swiglu_bwd(n, a, b, g, dt, dg, du, st)  # noqa: E731
    assert sb(a=None) == E and sb(b=None) == E and sb(g=None) == E and sb(dg=None) == E and sb(du=None) == E and sb(n=-1) == E and sb(dt=5) == E
    assert sb(n=0, a=None, b=None, g=None, dg=None, du=None) == 0
    torch.cuda.synchronize()
    assert bool((buf == CANARY).all())
