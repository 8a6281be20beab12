"""Packed varlen attention (pipelinerl_amd.fused_attention) against torch's scaled_dot_product_attention the way transformers'
sdpa path calls it, bf16, forward and backward, at the attention shapes of a Qwen2.5-0.5B micro-batch (2048 tokens, 14 query heads
on 2 KV heads, D = 64) and a Qwen2.5-7B one (8192 tokens, 28 on 4, D = 128), each as 1 sequence and as 8 equal sequences.

    fused              varlen_attention with the segment table
    sdpa_is_causal     no mask, is_causal=True: the fastest stock path.  It attends the row as ONE sequence - wrong for the
                       8-sequence cases, shown for scale
    sdpa_dense_mask    the [1, 1, N, N] block-diagonal causal bool mask (keys and values repeated to the query heads, as
                       transformers does when a mask is given): the only correct stock form for packed input

Per case and implementation: microseconds by HIP events (10 warm-ups, median of the iterations, the implementations alternating
in blocks in one process), FLOP/s counted on the VISIBLE score entries only (forward 4 D, backward 10 D per entry and query head),
the run-to-run spread ((p90 - p10) / median of forward + backward), and the peak of allocated bytes over one forward + backward
above what is allocated before it (inputs, upstream gradient, and for the dense form its mask).

Every case runs in a child process of its own under a time limit; the first one that fails or runs out of time ends the run.

    python scripts/attention_kernels_bench.py [--out profiles/attention_kernels_bench.json] [--iters 50] [--case-timeout 240]
"""

import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

CASES = {  # name -> (N, Hq, Hkv, D, sequences)
    "n2048_h14x2_d64_seq1": (2048, 14, 2, 64, 1),
    "n2048_h14x2_d64_seq8": (2048, 14, 2, 64, 8),
    "n8192_h28x4_d128_seq1": (8192, 28, 4, 128, 1),
    "n8192_h28x4_d128_seq8": (8192, 28, 4, 128, 8),
}


def run_case(name: str, iters: int) -> dict:
    import torch
    import torch.nn.functional as F

    from pipelinerl_amd import fused_attention as fa

    assert torch.cuda.is_available(), "this benchmark needs a HIP device"
    n, hq, hkv, d, seqs = CASES[name]
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device="cpu").manual_seed(1)
    mk = lambda *shape: torch.randn(*shape, generator=gen).to(torch.bfloat16).to(dev)  # noqa: E731
    # token-major memory, handed over as the [1, H, N, D] views a decoder layer makes of its projections
    q, k, v = mk(1, n, hq, d).requires_grad_(True), mk(1, n, hkv, d).requires_grad_(True), mk(1, n, hkv, d).requires_grad_(True)
    g = mk(1, n, hq, d)
    length = n // seqs
    pos = torch.arange(length, device=dev).repeat(seqs).view(1, n)
    ss, se = fa.segments(pos)
    scale = d ** -0.5
    visible = seqs * length * (length + 1) // 2
    flops = {"forward": 4 * d * visible * hq, "backward": 10 * d * visible * hq}
    mask = fa.block_diagonal_mask(ss, 1, n)
    rep = hq // hkv

    def fused():
        return fa.varlen_attention(q[0], k[0], v[0], ss, se, scale)[None]

    def sdpa_is_causal():
        qh, kh, vh = q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)
        return F.scaled_dot_product_attention(qh, kh, vh, is_causal=True, scale=scale, enable_gqa=True).transpose(1, 2)

    def sdpa_dense_mask():
        qh = q.transpose(1, 2)
        kh, vh = (t.transpose(1, 2).repeat_interleave(rep, dim=1) for t in (k, v))
        return F.scaled_dot_product_attention(qh, kh, vh, attn_mask=mask, scale=scale).transpose(1, 2)

    impls = {"fused": fused, "sdpa_is_causal": sdpa_is_causal, "sdpa_dense_mask": sdpa_dense_mask}
    leaves = [q, k, v]

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

    with torch.no_grad():  # the two correct forms agree (and with one sequence all three do)
        ref = sdpa_dense_mask().float()
        err = (fused().float() - ref).abs().max().item()
        assert err < 0.05, f"fused and dense-mask sdpa disagree by {err}"
    for fn in impls.values():  # warm: code objects, the allocator's blocks
        for _ in range(10):
            once(fn, None)
    torch.cuda.synchronize()
    events = {key: [] for key in impls}
    block = max(1, iters // 5)
    done = 0
    while done < iters:  # the implementations alternate in blocks: what shares the machine with this run hits all of them
        for key, fn in impls.items():
            for _ in range(block):
                once(fn, events[key])
        done += block
    torch.cuda.synchronize()
    res = {"case": name, "tokens": n, "query_heads": hq, "kv_heads": hkv, "head_size": d, "sequences": seqs, "dtype": "bf16", "iters": done,
           "visible_score_entries_per_head": visible, "flops_on_visible_entries": flops, "fused_vs_dense_mask_max_abs": err,
           "dense_mask_bytes": mask.numel() * mask.element_size()}
    for key, ev in events.items():
        fwd = statistics.median(a.elapsed_time(b) for a, b, _ in ev) * 1e3
        bwd = statistics.median(b.elapsed_time(c) for _, b, c in ev) * 1e3
        both_all = sorted(a.elapsed_time(c) * 1e3 for a, _, c in ev)
        both = statistics.median(both_all)
        p10, p90 = both_all[len(both_all) // 10], both_all[(9 * len(both_all)) // 10]
        res[key] = {"forward_us": fwd, "backward_us": bwd, "forward_backward_us": both, "forward_backward_p10_us": p10, "forward_backward_p90_us": p90,
                    "spread": (p90 - p10) / both, "forward_tflops_visible": flops["forward"] / fwd * 1e-6, "backward_tflops_visible": flops["backward"] / bwd * 1e-6,
                    "peak_allocated_bytes_forward_backward": peak(impls[key])}
    f, dm = res["fused"], res["sdpa_dense_mask"]
    res["fused_faster_than_dense_mask_by_more_than_the_spread"] = f["forward_backward_p90_us"] < dm["forward_backward_p10_us"]
    res["fused_over_is_causal_forward_backward"] = f["forward_backward_us"] / res["sdpa_is_causal"]["forward_backward_us"]
    # out, lse, delta and the three gradients: a small multiple of the bytes of q, k, v whatever N is
    res["qkv_bytes"] = 2 * n * d * (hq + 2 * hkv)
    res["fused_peak_over_qkv_bytes"] = f["peak_allocated_bytes_forward_backward"] / res["qkv_bytes"]
    res["fused_peak_has_no_n_squared_term"] = f["peak_allocated_bytes_forward_backward"] <= 3 * res["qkv_bytes"]
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
