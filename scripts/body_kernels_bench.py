"""Fused RMSNorm / SwiGLU (pipelinerl_amd.fused_body) against the stock eager modules of transformers, bf16, forward and backward,
at the shapes of a Qwen2.5-7B micro-batch (8192 tokens) and a Qwen2.5-0.5B one (1490 tokens).

Per case and implementation: microseconds by HIP events (warm, median over the iterations, the two implementations alternating
in blocks), the bytes the algorithm has to move, their share of 8 TB/s, and the peak of allocated bytes over one forward +
backward above what is allocated before it (inputs and the upstream gradient).

Every case runs in a child process of its own under a time limit; the first one that fails or runs out of time ends the run.

    python scripts/body_kernels_bench.py [--out profiles/body_kernels_bench.json] [--iters 50] [--case-timeout 240]
"""

import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

CASES = {
    "rmsnorm_8192x3584": ("rmsnorm", 8192, 3584),
    "rmsnorm_1490x896": ("rmsnorm", 1490, 896),
    "swiglu_8192x18944": ("swiglu", 8192, 18944),
    "swiglu_1490x4864": ("swiglu", 1490, 4864),
}
HBM_BYTES_PER_S = 8e12
EPS = 1e-6


def algorithmic_bytes(op: str, rows: int, cols: int) -> dict:
    n = rows * cols
    if op == "rmsnorm":  # x -> out (+ weight, rstd); x, g -> dx (+ weight, rstd, dw)
        return {"forward": 2 * n + 2 * n + 2 * cols + 4 * rows, "backward": 3 * 2 * n + 2 * cols + 4 * rows + 4 * cols}
    return {"forward": 3 * 2 * n, "backward": 5 * 2 * n}


def run_case(name: str, iters: int) -> dict:
    import torch
    from transformers.activations import ACT2FN
    from transformers.models.qwen2.modeling_qwen2 import Qwen2RMSNorm

    from pipelinerl_amd import fused_body

    assert torch.cuda.is_available(), "this benchmark needs a HIP device"
    op, rows, cols = CASES[name]
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device="cpu").manual_seed(1)
    mk = lambda *shape: torch.randn(*shape, generator=gen).to(torch.bfloat16).to(dev)  # noqa: E731
    g = mk(rows, cols)
    if op == "rmsnorm":
        x = mk(rows, cols).requires_grad_(True)
        norm = Qwen2RMSNorm(cols, eps=EPS).to(dev).to(torch.bfloat16)
        with torch.no_grad():
            norm.weight.copy_(1.0 + 0.25 * mk(cols))
        leaves = [x, norm.weight]
        impls = {"fused": lambda: fused_body.rms_norm(x, norm.weight, EPS), "eager": lambda: norm(x)}
    else:
        gate, up = mk(rows, cols).requires_grad_(True), mk(rows, cols).requires_grad_(True)
        act = ACT2FN["silu"]
        leaves = [gate, up]
        impls = {"fused": lambda: fused_body.swiglu(gate, up), "eager": lambda: act(gate) * up}

    def clear():
        for t in leaves:
            t.grad = None

    def once(fn, times):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        out = fn()
        e[1].record()
        out.backward(g)
        e[2].record()
        clear()
        if times is not None:
            times.append(e)

    def peak(fn):
        clear()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        once(fn, None)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    for fn in impls.values():  # warm: code objects, the allocator's blocks
        for _ in range(10):
            once(fn, None)
    torch.cuda.synchronize()
    events = {k: [] for k in impls}
    block = max(1, iters // 5)
    done = 0
    while done < iters:  # fused and eager alternate in blocks: what shares the machine with this run hits both
        for k, fn in impls.items():
            for _ in range(block):
                once(fn, events[k])
        done += block
    torch.cuda.synchronize()
    nbytes = algorithmic_bytes(op, rows, cols)
    res = {"case": name, "op": op, "rows": rows, "cols": cols, "dtype": "bf16", "iters": done, "algorithmic_bytes": nbytes}
    for k, ev in events.items():
        fwd = statistics.median(a.elapsed_time(b) for a, b, _ in ev) * 1e3
        bwd = statistics.median(b.elapsed_time(c) for _, b, c in ev) * 1e3
        both = statistics.median(a.elapsed_time(c) for a, _, c in ev) * 1e3
        res[k] = {"forward_us": fwd, "backward_us": bwd, "forward_backward_us": both,
                  "forward_share_of_8TBs": nbytes["forward"] / (fwd * 1e-6) / HBM_BYTES_PER_S,
                  "backward_share_of_8TBs": nbytes["backward"] / (bwd * 1e-6) / HBM_BYTES_PER_S,
                  "peak_allocated_bytes_forward_backward": peak(impls[k])}
    res["fused_faster_forward_backward"] = res["fused"]["forward_backward_us"] < res["eager"]["forward_backward_us"]
    return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default=None, help="run this one case in this process and print its JSON line")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--case-timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.case:
        print("RESULT " + json.dumps(run_case(a.case, a.iters)), flush=True)
        return 0
    results = []
    for name in CASES:
        try:
            p = subprocess.run([sys.executable, __file__, "--case", name, "--iters", str(a.iters)], capture_output=True, text=True, timeout=a.case_timeout)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {a.case_timeout} s; stopping here", flush=True)
            return 124
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            print(f"{name}: exit status {p.returncode}; stopping here\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", flush=True)
            return p.returncode or 1
        res = json.loads(lines[-1][len("RESULT "):])
        print(json.dumps(res), flush=True)
        results.append(res)
        if a.out:
            Path(a.out).write_text("\n".join(json.dumps(r) for r in results) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
