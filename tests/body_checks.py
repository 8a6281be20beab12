"""Per-entry checks of the fused body ops - RMSNorm and SwiGLU, forward and backward (plain torch; no kernel runs here).  The
scheme of tests/head_grad_checks.py: an fp64 witness, the size of each entry's own terms as its scale, and

    err = max over entries with scale > 0 of  max(|got - want| - out_rounding |want|, 0) / scale

`got` must be exactly 0 wherever scale == 0 (NaN counts as non-zero).  `out_rounding` is 2^-8 for a result delivered in bf16
(round-to-nearest keeps 8 significant bits: a worst case by construction, so it gets no factor) and 0 for fp32.

RMSNorm, x [R, H], weight w [H], upstream g [R, H], all as stored:
    rstd = 1 / sqrt(mean_H(x^2) + eps)      xh = x rstd
    out  = w xh                              scale |out|                       (rstd itself: scale |rstd|)
    dx   = rstd (g w - xh mean_H(g w xh))    scale rstd (|g w| + |xh| mean_H |g w xh|)
    dw   = sum_rows g xh                     scale sum_rows |g xh|
SwiGLU, s = sigmoid(gate):
    out    = silu(gate) up                   scale |out|
    d_up   = g silu(gate)                    scale |g silu|
    d_gate = g up s (1 + gate (1 - s))       scale |g up| (|s| + |s gate (1 - s)|)

Bounds.  bound = 4 x BODY_REF[op][output].  BODY_REF is the same metric for the REFERENCE op sequence - the formulas of the
installed transformers' Qwen2RMSNorm.forward and Qwen2MLP's `act_fn(gate) * up` (`reference_rmsnorm`, `reference_swiglu`: torch
CPU, fp32 arithmetic, autograd for the backward) on bf16-exact inputs - the largest value over the case family below, measured
on the CPU (tests/test_body_checks_host.py re-measures it), rounded up to two digits.  4 x is the project's standing margin for
a different summation order and 1-2 ulp of hardware exp / rsqrt.  No bound comes from a kernel; the kernels' values are in
DESIGN.md section 3b.  The fused ops are NOT bit-equal to eager bf16, which rounds the normalised tensor to bf16 before the
weight multiply: they are closer to the fp64 function.

Inputs never let a product of two stored values fall below the normal range of fp32 (the metric has no allowance for a flushed
or denormal product): the tiny row of the RMSNorm cases is 1e-20 x (its squares vanish against eps, nothing else is squared);
`up` and `g` of the SwiGLU edge case lie in [0.5, 2).
"""

from __future__ import annotations

import dataclasses

import torch
import torch.nn.functional as F

BF16_ROUNDING = 2.0 ** -8
EPS = 1e-6  # rms_norm_eps of the Qwen2.5 family

# op -> output -> largest value of the metric for the reference's fp32 arithmetic over the case family (CPU, torch 2.10)
BODY_REF = {
    "rmsnorm": {"out": 2.5e-7, "rstd": 1.8e-7, "dx": 3.6e-7, "dw": 2.7e-7},
    "swiglu": {"out": 1.9e-7, "d_gate": 8.0e-7, "d_up": 1.9e-7},  # d_gate: the 1490 x 4864 case (torch's 1 - sigmoid cancels for large gates)
}


def bound(op: str, output: str) -> float:
    return 4.0 * BODY_REF[op][output]


def out_rounding(dtype) -> float:
    return BF16_ROUNDING if dtype == torch.bfloat16 else 0.0


# ---- the case family ---------------------------------------------------------------------------------------------------------
def rmsnorm_cols(geom: dict, x_bf16: bool) -> list[int]:
    """H at the kernels' edges: below / at / past one vector, one vector short of / exactly / one element past a wave's width
    (64 lanes x V) and a workgroup's (256 threads x V), and the hidden sizes of Qwen2.5 0.5B / 7B / 14B."""
    v = geom["vec_bf16"] if x_bf16 else geom["vec_f32"]
    wave, block = geom["wave"] * v, geom["block"] * v
    return sorted({1, 7, 8, 9, wave - v, wave, wave + 1, block - v, block, block + 1, 896, 3584, 5120})


def rmsnorm_rows(geom: dict) -> list[int]:
    b = geom["band_rows"]
    return [1, 2, b - 1, b, b + 1, 2 * b + 1]


def swiglu_numels(geom: dict) -> list[int]:
    n = geom["block"] * geom["swiglu_vec"]
    return [1, 7, 8, 9, n - 1, n, n + 1]


SWIGLU_MODEL_SHAPE = (1490, 4864)  # a 1490-token micro-batch of Qwen2.5-0.5B
GATE_EDGES = (0.0, 1e-30, -1e-30, 20.0, -20.0, 88.0, -88.0)


def bf16_exact(t: torch.Tensor) -> torch.Tensor:
    return t.float().to(torch.bfloat16).float()


def rmsnorm_inputs(rows: int, cols: int, seed: int | None = None, special: bool = False):
    """(x, w, g) fp32 tensors holding bf16-exact values: rows of standard deviation 0.1 .. 10, w = 1 + randn / 4, g = randn.
    `special` (rows >= 3): row 1 is all zeros, row 2 is scaled by 1e-20 (its variance is far below eps)."""
    gen = torch.Generator().manual_seed(rows * 100003 + cols if seed is None else seed)
    x = torch.randn(rows, cols, generator=gen) * torch.exp(torch.empty(rows, 1).uniform_(-2.3, 2.3, generator=gen))
    w = 1.0 + 0.25 * torch.randn(cols, generator=gen)
    g = torch.randn(rows, cols, generator=gen)
    if special:
        x[1] = 0.0
        x[2] *= 1e-20
    return bf16_exact(x), bf16_exact(w), bf16_exact(g)


def swiglu_inputs(numel: int, seed: int | None = None, edges: bool = False):
    """(gate, up, g) fp32, bf16-exact: gate = 3 randn.  `edges`: gate cycles through GATE_EDGES, |up| and |g| in [0.5, 2)."""
    gen = torch.Generator().manual_seed(numel if seed is None else seed)
    gate = 3.0 * torch.randn(numel, generator=gen)
    up = torch.randn(numel, generator=gen)
    g = torch.randn(numel, generator=gen)
    if edges:
        gate = torch.tensor(GATE_EDGES).repeat(-(-numel // len(GATE_EDGES)))[:numel]
        sign = lambda t: torch.where(t < 0, -torch.ones_like(t), torch.ones_like(t))  # noqa: E731
        up = sign(up) * torch.empty(numel).uniform_(0.5, 2.0, generator=gen)
        g = sign(g) * torch.empty(numel).uniform_(0.5, 2.0, generator=gen)
    return bf16_exact(gate), bf16_exact(up), bf16_exact(g)


# ---- witnesses (fp64) --------------------------------------------------------------------------------------------------------
def rmsnorm_witness(x, w, g, eps: float = EPS) -> dict:
    """output -> (want, scale), fp64, for x [R, H], w [H], g [R, H] as stored."""
    x, w, g = x.detach().double().cpu(), w.detach().double().cpu(), g.detach().double().cpu()
    rstd = 1.0 / torch.sqrt((x * x).mean(-1, keepdim=True) + eps)
    xh = x * rstd
    gw = g * w
    out = w * xh
    dx = rstd * (gw - xh * (gw * xh).mean(-1, keepdim=True))
    s_dx = rstd * (gw.abs() + xh.abs() * (gw * xh).abs().mean(-1, keepdim=True))
    return {"out": (out, out.abs()), "rstd": (rstd[:, 0], rstd[:, 0].abs()), "dx": (dx, s_dx),
            "dw": ((g * xh).sum(0), (g * xh).abs().sum(0))}


def swiglu_witness(gate, up, g) -> dict:
    z, up, g = gate.detach().double().cpu(), up.detach().double().cpu(), g.detach().double().cpu()
    s = torch.sigmoid(z)
    silu = z * s
    out = silu * up
    return {"out": (out, out.abs()), "d_up": (g * silu, (g * silu).abs()),
            "d_gate": (g * up * s * (1.0 + z * (1.0 - s)), (g * up).abs() * (s.abs() + (s * z * (1.0 - s)).abs()))}


# ---- the reference op sequences, fp32 ------------------------------------------------------------------------------------------
def reference_rmsnorm(x, w, g, eps: float = EPS) -> dict:
    """Qwen2RMSNorm.forward of the installed transformers in fp32 (the casts are no-ops), backward by autograd."""
    x = x.detach().float().clone().requires_grad_(True)
    w = w.detach().float().clone().requires_grad_(True)
    hidden = x.to(torch.float32)
    variance = hidden.pow(2).mean(-1, keepdim=True)
    rstd = torch.rsqrt(variance + eps)
    out = w * (hidden * rstd).to(x.dtype)
    out.backward(g.detach().float())
    return {"out": out.detach(), "rstd": rstd.detach()[:, 0], "dx": x.grad, "dw": w.grad}


def reference_swiglu(gate, up, g) -> dict:
    gate = gate.detach().float().clone().requires_grad_(True)
    up = up.detach().float().clone().requires_grad_(True)
    out = F.silu(gate) * up
    out.backward(g.detach().float())
    return {"out": out.detach(), "d_gate": gate.grad, "d_up": up.grad}


# ---- the functions restated in fp64, with seeded mistakes (what the host test shows the bounds catch) ---------------------------
def restated_rmsnorm(x, w, g, eps: float = EPS, mistake: str | None = None, band_rows: int = 32) -> dict:
    x, w, g = x.double(), w.double(), g.double()
    cols = x.shape[-1]
    ss = (x * x).sum(-1, keepdim=True)
    var = ss / (cols - 1 if mistake == "mean_over_h_minus_1" else cols)
    rstd = 1.0 / torch.sqrt(var if mistake == "eps_dropped" else var + eps)
    xh = x * rstd
    gw = g * w
    c = (gw * xh).mean(-1, keepdim=True)
    dx = rstd * gw if mistake == "dx_mean_term_dropped" else rstd * (gw - xh * c)
    rows = x.shape[0]
    last = ((rows - 1) // band_rows) * band_rows
    dw = (g * xh)[:last].sum(0) if mistake == "dw_last_band_missing" else (g * xh).sum(0)
    return {"out": w * xh, "rstd": rstd[:, 0], "dx": dx, "dw": dw}


def restated_swiglu(gate, up, g, mistake: str | None = None) -> dict:
    z, up, g = gate.double(), up.double(), g.double()
    s = torch.sigmoid(z)
    inner = torch.ones_like(z) if mistake == "d_gate_term_dropped" else 1.0 + z * (1.0 - s)
    return {"out": z * s * up, "d_up": g * z * s, "d_gate": g * up * s * inner}


RMSNORM_MISTAKES = ("eps_dropped", "mean_over_h_minus_1", "dx_mean_term_dropped", "dw_last_band_missing")
SWIGLU_MISTAKES = ("d_gate_term_dropped",)


# ---- the metric --------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class BodyCheck:
    output: str
    err: float          # max over entries with scale > 0 of the excess error / scale
    index: tuple        # of the worst entry
    got: float
    want: float
    scale: float
    stray: int          # non-zero entries where scale == 0 (must be 0)
    stray_at: tuple | None

    def __str__(self):
        s = f"per-entry {self.output} error {self.err:.3e} at {self.index}: got {self.got:.9e} want {self.want:.9e} scale {self.scale:.3e}"
        if self.stray:
            s += f"; {self.stray} non-zero entries where the result is exactly 0, first at {self.stray_at}"
        return s

    def ok(self, limit: float) -> bool:
        return self.stray == 0 and self.err <= limit  # NaN fails


def measure(output: str, got, want, scale, rounding: float = 0.0) -> BodyCheck:
    got = got.detach().double().cpu().reshape(want.shape)
    live = scale > 0
    bad = ~live & (got != 0)  # NaN != 0 is true
    stray = int(bad.sum())
    stray_at = tuple(bad.nonzero()[0].tolist()) if stray else None
    e = ((got - want).abs() - rounding * want.abs()).clamp_min(0.0) / torch.where(live, scale, torch.ones_like(scale))
    e = torch.where(live, e, torch.zeros_like(e))
    e = torch.where(~torch.isfinite(got) & live, torch.full_like(e, float("inf")), e)
    if e.numel() == 0:
        return BodyCheck(output, 0.0, (), 0.0, 0.0, 0.0, stray, stray_at)
    k = int(e.argmax())
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(k), e.shape))
    return BodyCheck(output, float(e.flatten()[k]), idx, float(got.flatten()[k]), float(want.flatten()[k]), float(scale.flatten()[k]), stray, stray_at)


def check_outputs(op: str, label: str, got: dict, witness: dict, rounding: dict | None = None, verbose: bool = True) -> dict:
    """Every output of `got` against the witness under bound(op, output); prints each figure before it asserts.
    `rounding`: output -> out_rounding (default 0).  Returns output -> err."""
    errs, failed = {}, []
    for name, value in got.items():
        want, scale = witness[name]
        res = measure(name, value, want, scale, (rounding or {}).get(name, 0.0))
        errs[name] = res.err
        if verbose:
            print(f"[body] {op} {label}: {res} (bound {bound(op, name):.2e})")
        if not res.ok(bound(op, name)):
            failed.append(str(res) + f" > bound {bound(op, name):.3e}")
    assert not failed, f"{op} {label}: " + "; ".join(failed)
    return errs
