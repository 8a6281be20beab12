"""The slice form of the packed attention kernels (csrc/prl_attention_sp.hip) against the square kernels on the same row, in ONE
process on one GPU: what the sequence-parallel form costs in kernel time before any byte crosses a wire.

A row of 8192 tokens (28 query heads on 4 KV heads, D = 128: a Qwen2.5-7B layer), as 1 sequence and as 8 equal sequences, cut
into P = 2 and P = 4 slices.  Per case:

    square    varlen_attention forward + backward on the whole row (bf16 dK / dV written once)
    sliced    the P slices one after the other - what the P ranks would run side by side - forward, backward (fp32 dK / dV
              partials over the WHOLE row per slice) and the fold of the P partials of dK and of dV; reported as the SUM over the
              slices, and the longest single slice (the last one: causal work is not balanced across ranks)

The matrix work of the two forms is the same; the difference is the fp32 partial stores (2 x 4 x N Hkv D bytes per slice) and the
fold.  Microseconds by HIP events, 10 warm-ups, the median of the iterations, the two forms alternating in blocks.  The exchange
itself (all-gather of K / V, all-to-all of the partials) needs a second GPU and is not measured here: only its bytes are stated.

    python scripts/attention_sp_kernels_bench.py [--out profiles/attention_sp_kernels_bench.json] [--iters 50] [--case-timeout 240]
"""

import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SHAPE = (8192, 28, 4, 128)  # N, Hq, Hkv, D
CASES = {f"n8192_h28x4_d128_seq{seqs}_p{p}": (seqs, p) for seqs in (1, 8) for p in (2, 4)}


def run_case(name: str, iters: int) -> dict:
    import torch

    from pipelinerl_amd import fused_attention as fa

    assert torch.cuda.is_available(), "this benchmark needs a HIP device"
    n, hq, hkv, d = SHAPE
    seqs, p = CASES[name]
    length = n // p
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device="cpu").manual_seed(1)
    mk = lambda *shape: torch.randn(*shape, generator=gen).to(torch.bfloat16).to(dev)  # noqa: E731
    q, k, v, g = mk(n, hq, d), mk(n, hkv, d), mk(n, hkv, d), mk(n, hq, d)
    ss, se = fa.segments(torch.arange(n // seqs, device=dev).repeat(seqs).view(1, n))
    scale = d ** -0.5
    qs = [q[r * length:(r + 1) * length] for r in range(p)]
    gs = [g[r * length:(r + 1) * length] for r in range(p)]
    parts_k = torch.zeros(p, n * hkv * d, dtype=torch.float32, device=dev)  # what a rank holds after the all-to-all: P pieces of its rows
    parts_v = torch.zeros_like(parts_k)

    def ev():
        return torch.cuda.Event(enable_timing=True)

    def square(times):
        ql, kl, vl = (t.detach().requires_grad_(True) for t in (q, k, v))
        e = [ev() for _ in range(3)]
        e[0].record()
        out = fa.varlen_attention(ql, kl, vl, ss, se, scale)
        e[1].record()
        out.backward(g)
        e[2].record()
        if times is not None:
            times.append({"forward": (e[0], e[1]), "backward": (e[1], e[2])})
        return out.detach(), ql.grad, kl.grad, vl.grad

    def sliced(times):
        rec = {"forward": [], "backward": []}
        saved = []
        for r in range(p):
            a, b = ev(), ev()
            a.record()
            saved.append(fa._slice_forward(qs[r], k, v, ss, se, r * length, scale))
            b.record()
            rec["forward"].append((a, b))
        grads = []
        for r in range(p):
            a, b = ev(), ev()
            a.record()
            grads.append(fa._slice_backward(qs[r], k, v, ss, se, r * length, scale, saved[r][0], saved[r][1], gs[r]))
            b.record()
            rec["backward"].append((a, b))
        a, b = ev(), ev()
        a.record()
        dk, dv = fa.fold_parts(parts_k), fa.fold_parts(parts_v)  # P folds of 1 / P of the row each = one fold of the row
        b.record()
        rec["fold"] = [(a, b)]
        if times is not None:
            times.append(rec)
        return saved, grads, dk, dv

    # the two forms agree: out and dq of the slices at a multiple of 64 bit for bit, the folded dk / dv to the 4 x margin's order
    out, dq, dk, dv = square(None)
    saved, grads, _, _ = sliced(None)
    torch.cuda.synchronize()
    assert length % 64 == 0
    for r in range(p):
        rows = slice(r * length, (r + 1) * length)
        assert torch.equal(saved[r][0], out[rows]) and torch.equal(grads[r][0], dq[rows]), f"slice {r} differs from the square kernels"
        parts_k[r].copy_(grads[r][1].view(-1))
        parts_v[r].copy_(grads[r][2].view(-1))
    fk, fv = fa.fold_parts(parts_k).view(n, hkv, d), fa.fold_parts(parts_v).view(n, hkv, d)
    diff = max((fk.float() - dk.float()).abs().max().item() / dk.float().abs().max().item(),
               (fv.float() - dv.float()).abs().max().item() / dv.float().abs().max().item())
    assert diff < 2.0 ** -6, f"folded dk / dv differ from the square kernels' by {diff}"
    del saved, grads

    for fn in (square, sliced):
        for _ in range(10):
            fn(None)
    torch.cuda.synchronize()
    events = {"square": [], "sliced": []}
    block = max(1, iters // 5)
    done = 0
    while done < iters:
        for key, fn in (("square", square), ("sliced", sliced)):
            for _ in range(block):
                fn(events[key])
        done += block
    torch.cuda.synchronize()

    def us(pair):
        return pair[0].elapsed_time(pair[1]) * 1e3

    med = statistics.median
    sq = {ph: med(us(t[ph]) for t in events["square"]) for ph in ("forward", "backward")}
    sl = {ph: med(sum(us(x) for x in t[ph]) for t in events["sliced"]) for ph in ("forward", "backward", "fold")}
    last = {ph: med(us(t[ph][-1]) for t in events["sliced"]) for ph in ("forward", "backward")}
    sq_total = med(us(t["forward"]) + us(t["backward"]) for t in events["square"])
    sl_all = sorted(sum(us(x) for ph in ("forward", "backward", "fold") for x in t[ph]) for t in events["sliced"])
    sl_total = med(sl_all)
    kv_bytes = 2 * n * hkv * d * 2
    return {"case": name, "tokens": n, "query_heads": hq, "kv_heads": hkv, "head_size": d, "sequences": seqs, "slices": p, "iters": done,
            "square_us": {**sq, "forward_backward": sq_total},
            "sliced_sum_us": {**sl, "forward_backward_fold": sl_total, "p10": sl_all[len(sl_all) // 10], "p90": sl_all[(9 * len(sl_all)) // 10]},
            "last_slice_us": last,
            "sliced_over_square": sl_total / sq_total,
            "folded_dkdv_vs_square_max_rel": diff,
            "bytes_per_layer": {"kv_gathered_per_rank": kv_bytes, "partials_per_rank_fp32": 2 * kv_bytes, "saved_gathered_kv_per_rank": kv_bytes},
            "exchange_us": None}


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
