"""Fused body ops: the RMSNorm and SwiGLU of every decoder layer as single HIP launches (csrc/prl_body.hip).

The learner's micro-batch at 0.5B is host-issue bound, and the two elementwise / row-reduce chains of a decoder layer are
where the launches are: transformers' `Qwen2RMSNorm.forward` is 8 eager launches (to fp32, pow, mean, + eps, rsqrt, mul,
to bf16, weight *) and about a dozen in backward; `act_fn(gate) * up` is 2 and 3.  Here

    rms_norm(x, weight, eps)   1 launch forward (out, rstd), 2 backward (dx with dw's partials per 32-row band; their fold)
    swiglu(gate, up)           1 launch forward, 1 backward

Memory: eager RMSNorm keeps `x.float()` (4 B / element) and the bf16 normalised tensor (2 B / element) for its backward; the
fused form keeps x itself (which the surrounding graph holds anyway), the weight and `rstd`, 4 B per ROW.  SwiGLU keeps gate
and up and not the `silu(gate)` intermediate.

Numerics: everything is computed in fp32 from the stored values and rounded once.  Eager bf16 rounds the normalised tensor to
bf16 BEFORE the weight multiply, so the fused ops are not bit-equal to it - they are closer to the fp64 function
(tests/body_checks.py).

`install_fused_body(model)` patches the instance `forward` of the modules it recognises; it is opt-in, replaces no module and
touches no parameter.  Not covered: RoPE (`apply_rotary_pos_emb` is a module-level function of
transformers - patching it is process-global, not per model) and the residual add in front of a norm (owning it means owning
the decoder layer's forward).
"""

from __future__ import annotations

import ctypes
from typing import Any

import torch
from torch.autograd.function import once_differentiable

from . import _lib

_DTYPE_CODE = {torch.float32: _lib.PRL_DTYPE_F32, torch.bfloat16: _lib.PRL_DTYPE_BF16}

# classes with exactly the formula of the kernels: weight * (x * rsqrt(mean(x^2) + eps)), the product formed in fp32 ...
RMSNORM_CLASSES = ("Qwen2RMSNorm", "Qwen3RMSNorm", "LlamaRMSNorm", "MistralRMSNorm")
# ... and down_proj(act_fn(gate_proj(x)) * up_proj(x))
MLP_CLASSES = ("Qwen2MLP", "Qwen3MLP", "LlamaMLP", "MistralMLP")


def _supported(*tensors: torch.Tensor) -> bool:
    """The kernels take these tensors: on a HIP device, fp32 or bf16.  Anything else goes to the module's own forward."""
    return all(t.is_cuda and t.dtype in _DTYPE_CODE for t in tensors)


def _require(*tensors: torch.Tensor) -> None:
    for t in tensors:
        if not t.is_cuda:
            _lib.require_device(t)
        if t.dtype not in _DTYPE_CODE:
            raise TypeError(f"the fused body kernels take fp32 and bf16 tensors, not {t.dtype}")


# The learner's micro-batch is host-issue bound and these functions run 3 x layers times forward and again backward: what the
# interpreter does per call is kept short - the entry points are looked up once, the stream handle comes from torch's raw
# accessor, and the device guard is entered only for a tensor that is not on the current device.
_entry: dict[str, Any] = {}
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_ws_bytes: dict[tuple[int, int], int] = {}


def _fn(name: str):
    fn = _entry.get(name)
    if fn is None:
        fn = _entry[name] = getattr(_lib.load(), name)
    return fn


def _launch(name: str, device: torch.device, *args) -> None:
    """Call the entry point `name` with `args` + the current stream of `device`, on that device."""
    idx = device.index
    if idx is None or idx != torch.cuda.current_device():
        with torch.cuda.device(device):
            return _launch(name, torch.device("cuda", torch.cuda.current_device()), *args)
    rc = _fn(name)(*args, _raw_stream(idx) if _raw_stream is not None else _lib.current_stream_ptr(device))
    if rc:
        _lib.check(rc)


def _workspace_bytes(rows: int, cols: int) -> int:
    need = _ws_bytes.get((rows, cols))
    if need is None:
        out = ctypes.c_size_t(0)
        _lib.check(_fn("prl_rmsnorm_workspace_bytes")(rows, cols, ctypes.byref(out)))
        if len(_ws_bytes) > 4096:
            _ws_bytes.clear()
        need = _ws_bytes[(rows, cols)] = out.value
    return need


class _RmsNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, eps):  # type: ignore[override]
        _require(x, weight)
        cols = x.shape[-1]
        if weight.dim() != 1 or weight.shape[0] != cols:
            raise ValueError(f"weight {tuple(weight.shape)} does not match the last dimension of x {tuple(x.shape)}")
        xc, wc = x.contiguous(), weight.contiguous()
        rows = xc.numel() // cols if cols else 0
        out = torch.empty(x.shape, dtype=xc.dtype if xc.dtype == wc.dtype else torch.float32, device=x.device)
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
        _launch("prl_rmsnorm_fwd", x.device, rows, cols, xc.data_ptr(), _DTYPE_CODE[xc.dtype], wc.data_ptr(), _DTYPE_CODE[wc.dtype], float(eps),
                out.data_ptr(), rstd.data_ptr())
        ctx.save_for_backward(xc, wc, rstd)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):  # type: ignore[override]
        xc, wc, rstd = ctx.saved_tensors
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_x or need_w):
            return None, None, None
        cols = xc.shape[-1]
        rows = rstd.shape[0]
        g = grad_out.contiguous()
        dx = torch.empty_like(xc) if need_x else None
        dw = ws = None
        ws_bytes = 0
        if need_w:
            dw = torch.empty(cols, dtype=torch.float32, device=xc.device)
            ws_bytes = _workspace_bytes(rows, cols)
            ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=xc.device)
        _launch("prl_rmsnorm_bwd", xc.device, rows, cols, xc.data_ptr(), _DTYPE_CODE[xc.dtype], wc.data_ptr(), _DTYPE_CODE[wc.dtype], rstd.data_ptr(),
                g.data_ptr(), _lib.ptr(dx), _lib.ptr(dw), _lib.ptr(ws), ws_bytes)
        if need_w and wc.dtype != torch.float32:
            dw = dw.to(wc.dtype)
        return dx, dw, None


class _SwigluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gate, up):  # type: ignore[override]
        _require(gate, up)
        if gate.shape != up.shape or gate.dtype != up.dtype:
            raise ValueError(f"gate {tuple(gate.shape)} {gate.dtype} and up {tuple(up.shape)} {up.dtype} must agree in shape and dtype")
        gc, uc = gate.contiguous(), up.contiguous()
        out = torch.empty_like(gc)
        _launch("prl_swiglu_fwd", gc.device, gc.numel(), gc.data_ptr(), uc.data_ptr(), _DTYPE_CODE[gc.dtype], out.data_ptr())
        ctx.save_for_backward(gc, uc)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):  # type: ignore[override]
        gc, uc = ctx.saved_tensors
        g = grad_out.contiguous()
        d_gate, d_up = torch.empty_like(gc), torch.empty_like(uc)
        _launch("prl_swiglu_bwd", gc.device, gc.numel(), gc.data_ptr(), uc.data_ptr(), g.data_ptr(), _DTYPE_CODE[gc.dtype], d_gate.data_ptr(),
                d_up.data_ptr())
        return d_gate, d_up


def rms_norm(x: torch.Tensor, weight: torch.Tensor, eps: float) -> torch.Tensor:
    """`weight * (x * rsqrt(mean(x^2, -1) + eps))` over the last dimension of `x` (any leading shape; fp32 or bf16, the weight
    independently), computed in fp32 and rounded once to torch's promotion of (weight, x).  Differentiable in x and weight;
    saves x, weight and the per-row `rstd` only.  Raises on CPU tensors: there is no fallback here."""
    return _RmsNormFn.apply(x, weight, eps)


def swiglu(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    """`silu(gate) * up` (same shape and dtype, fp32 or bf16), in fp32, rounded once.  Saves gate and up only."""
    return _SwigluFn.apply(gate, up)


# ---- installation -----------------------------------------------------------------------------------------------------------
def _norm_problem(mod: Any) -> str | None:
    w = getattr(mod, "weight", None)
    if not isinstance(w, torch.Tensor) or w.dim() != 1:
        return "no 1-D weight"
    if not hasattr(mod, "variance_epsilon"):
        return "no variance_epsilon"
    return None


def _mlp_problem(mod: Any, model_config: Any) -> str | None:
    for name in ("gate_proj", "up_proj", "down_proj"):
        if getattr(mod, name, None) is None:
            return f"no {name}"
    act = getattr(getattr(mod, "config", None) or model_config, "hidden_act", None)
    if act != "silu":
        return f"config.hidden_act = {act!r}, the kernel computes silu"
    return None


def _patch_norm(mod: Any) -> None:
    original = mod.forward

    def forward(hidden_states, *args, **kwargs):
        if not args and not kwargs and _supported(hidden_states, mod.weight):
            return rms_norm(hidden_states, mod.weight, mod.variance_epsilon)
        return original(hidden_states, *args, **kwargs)

    mod._prl_fused_body_original = original
    mod.forward = forward


def _patch_mlp(mod: Any) -> None:
    original = mod.forward

    def forward(x, *args, **kwargs):
        if args or kwargs or not _supported(x):
            return original(x, *args, **kwargs)
        gate, up = mod.gate_proj(x), mod.up_proj(x)
        if not _supported(gate, up) or gate.dtype != up.dtype:  # (autocast to a dtype the kernels do not take)
            return mod.down_proj(mod.act_fn(gate) * up)
        return mod.down_proj(swiglu(gate, up))

    mod._prl_fused_body_original = original
    mod.forward = forward


def install_fused_body(model: Any, rmsnorm: bool = True, swiglu: bool = True) -> Any:
    """Route the RMSNorm and gated-MLP modules of a Hugging Face causal LM (bare or inside the actor-critic wrapper) through
    `rms_norm` / `swiglu`.  Only the instance `forward` of a recognised sub-module is patched: no module is replaced or renamed,
    `named_parameters()` and `state_dict()` are what they were, and `install_fused_head` composes in either order.

    Recognised: a module whose class is named in RMSNORM_CLASSES with a 1-D `weight` and a `variance_epsilon`; a module whose
    class is named in MLP_CLASSES with `gate_proj` / `up_proj` / `down_proj` and `config.hidden_act == "silu"`.  A module that
    looks like one of the two (class name ending in RMSNorm / Norm / MLP) but is not recognised is left alone and listed with
    the reason in `model._prl_fused_body = {"rmsnorm": n, "swiglu": m, "skipped": [(name, why), ...]}`.

    A patched forward calls the module's original forward for a tensor that is not on a HIP device or not fp32 / bf16, so
    the model may still be on the CPU when this runs.  Calling it again changes nothing."""
    from .fused_head import _lm_of

    report = getattr(model, "_prl_fused_body", None)
    if report is not None:
        return model
    lm = _lm_of(model)
    config = getattr(lm, "config", None)
    report = {"rmsnorm": 0, "swiglu": 0, "skipped": []}
    for name, mod in lm.named_modules():
        cls = type(mod).__name__
        if hasattr(mod, "_prl_fused_body_original"):  # patched through another handle on the same modules
            report["rmsnorm" if cls in RMSNORM_CLASSES else "swiglu"] += 1
            continue
        if cls in RMSNORM_CLASSES:
            why = _norm_problem(mod) if rmsnorm else "rmsnorm=False"
            if why is None:
                _patch_norm(mod)
                report["rmsnorm"] += 1
            else:
                report["skipped"].append((name, why))
        elif cls in MLP_CLASSES:
            why = _mlp_problem(mod, config) if swiglu else "swiglu=False"
            if why is None:
                _patch_mlp(mod)
                report["swiglu"] += 1
            else:
                report["skipped"].append((name, why))
        elif cls.endswith(("RMSNorm", "MLP")) or (cls.endswith("Norm") and not list(mod.children())):
            report["skipped"].append((name, f"class {cls} is not in the list of same-formula classes"))
    model._prl_fused_body = report
    return model
