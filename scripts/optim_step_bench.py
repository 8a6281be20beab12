"""Time the learner-step boundary on the Qwen2.5-7B parameter list (`weight_sync_probe.qwen25_shapes("7b")`): bf16 parameters
and gradients, the output head in fp32.

  torch            clip_grad_norm_ + float() + torch.optim.AdamW(fused=True).step()   (bf16 state; the boundary before FusedAdamW)
  fused            FusedAdamW.clip_and_step, master weights off                        (fp32 state, like for like in what is updated)
  fused_master     FusedAdamW.clip_and_step, master weights on                         (moves more bytes: + 8 B per bf16 element)

HIP events around every boundary, >= 20 timed boundaries after warm-up.  Every configuration runs in a child process of its
own under its own time limit; the first one that fails ends the run.  One JSON object on stdout and in --out.

    python scripts/optim_step_bench.py --out profiles/optim_step_bench.json

`--mode grad_accum` times the fp32 gradient fold on the same list instead (the bf16 parameters; the fp32 head bypasses the accumulator):

  fold_add         prl_optim_grad_accumulate, overwrite = 0: acc += g.float()         (2 + 4 read, 4 written = 10 B/element)
  fold_overwrite   prl_optim_grad_accumulate, overwrite = 1: acc = g.float()          (2 read, 4 written = 6 B/element)
  torch_add        per parameter `acc.add_(p.grad)` into preallocated fp32 tensors    (the stock equivalent of fold_add)

all three in ONE child process on the same gradients, HIP events around each repetition, 20 repetitions after warm-up, median [min, max].

    python scripts/optim_step_bench.py --mode grad_accum --out profiles/grad_accum_bench.json

`--mode adafactor` times the Adafactor boundary on the Qwen2.5-0.5B parameter list (bf16 parameters and gradients; the embeddings are tied, so there is no separate head):

  fused_adafactor  FusedAdafactor.clip_and_step, master weights on                    (norm 2 + step 2 + 2 + 2 + 4 read, 4 + 2 written = 18 B per bf16 element)
  transformers     clip_grad_norm_ + transformers.Adafactor(relative_step=False, scale_parameter=False).step() on a twin parameter set

both in ONE child process, alternating, HIP events around each boundary, 20 boundaries after warm-up, median [min, max].

    python scripts/optim_step_bench.py --mode adafactor --out profiles/adafactor_step_bench.json

`--mode compact` times the AdamW STEP alone (`step()`, coefficient 1, no norm pass) with compact state against the fp32-state step, on the
same parameters and gradients (the 7B list; each configuration has its own state):

  fp32_state         FusedAdamW(master_weights=False)                                   (optim_step_kernel: 22 B per bf16 element)
  fp32_state_master  FusedAdamW(master_weights=True)                                    (optim_step_kernel: 28 B)
  compact            FusedAdamW(master_weights=False, state_dtype=torch.bfloat16, param_rounding="stochastic")
                                                                                        (optim_step_compact_kernel: 14 B)

all three in ONE child process, alternating, HIP events around each step, 20 steps after warm-up, median [min, max].

    python scripts/optim_step_bench.py --mode compact --out profiles/optim_compact_step_bench.json
"""

from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

PEAK_GBS, COPY_CEILING_GBS = 8000.0, 6290.0
CONFIGS = ("torch", "fused", "fused_master")


def bytes_needed(shapes, config: str) -> int:
    total = 0
    for name, shape in shapes:
        n = 1
        for d in shape:
            n *= d
        e = 4 if name == "lm_head.weight" else 2
        state = {"torch": 2 * e, "fused": 8, "fused_master": 8 + (4 if e == 2 else 0)}[config]
        total += n * (2 * e + state)
    return total


def run_one(config: str, steps: int, warmup: int, max_norm: float) -> dict:
    import torch

    from pipelinerl_amd.finetune.optim import FusedAdamW
    from pipelinerl_amd.weight_sync_probe import qwen25_shapes

    dev = torch.device("cuda", 0)
    shapes = qwen25_shapes("7b")
    free, _ = torch.cuda.mem_get_info(dev)
    full = len(shapes)
    while bytes_needed(shapes, config) > 0.9 * free:  # the largest prefix of the list that fits
        shapes = shapes[:-1]
    params = []
    gen = torch.Generator(device=dev).manual_seed(0)
    for name, shape in shapes:
        dtype = torch.float32 if name == "lm_head.weight" else torch.bfloat16
        p = torch.nn.Parameter(torch.empty(shape, dtype=dtype, device=dev).normal_(0.0, 0.02, generator=gen))
        p.grad = torch.empty(shape, dtype=dtype, device=dev).normal_(0.0, 1e-3, generator=gen)
        params.append(p)
    numel = sum(p.numel() for p in params)
    if config == "torch":
        opt = torch.optim.AdamW(params, lr=1e-6, fused=True)

        def boundary():
            gn = torch.nn.utils.clip_grad_norm_(params, max_norm)
            float(gn)
            opt.step()
    else:
        opt = FusedAdamW(params, lr=1e-6, master_weights=config == "fused_master")

        def boundary():
            opt.clip_and_step(max_norm)

    times = []
    for k in range(warmup + steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        boundary()
        b.record()
        b.synchronize()
        if k >= warmup:
            times.append(a.elapsed_time(b))
    out = {"config": config, "tensors": len(params), "of_tensors": full, "numel": numel, "steps": steps, "warmup": warmup,
           "median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times)}
    if config != "torch":
        # algorithmic bytes: the norm pass reads every gradient once; the step reads g, weights, m, v and writes weights (+ the bf16
        # image under master weights), m, v
        alg = 0
        for p in params:
            e = p.element_size()
            master = config == "fused_master" and e == 2
            alg += p.numel() * (e + e + (4 if master else e) + 8 + (4 if master else 0) + e + 8)
        gbs = alg / (out["median_ms"] * 1e-3) / 1e9
        out.update(algorithmic_bytes=alg, achieved_gbs=gbs, frac_of_peak=gbs / PEAK_GBS, frac_of_copy_ceiling=gbs / COPY_CEILING_GBS)
    return out


def run_grad_accum(steps: int, warmup: int) -> dict:
    import torch

    from pipelinerl_amd import _lib
    from pipelinerl_amd.weight_sync_probe import qwen25_shapes

    dev = torch.device("cuda", 0)
    shapes = [(n, s) for n, s in qwen25_shapes("7b") if n != "lm_head.weight"]
    gen = torch.Generator(device=dev).manual_seed(0)
    grads = [torch.empty(shape, dtype=torch.bfloat16, device=dev).normal_(0.0, 1e-3, generator=gen) for _, shape in shapes]
    numel = sum(g.numel() for g in grads)
    slots = [(-(-g.numel() // 16)) * 16 for g in grads]
    flat = torch.zeros(sum(slots), dtype=torch.float32, device=dev)  # the optimizer's layout: one flat buffer, 64-byte aligned slots
    table = (_lib.PrlAccumSegment * len(grads))()
    off = 0
    for seg, g, slot in zip(table, grads, slots):
        seg.grad, seg.acc, seg.numel, seg.grad_dtype = g.data_ptr(), flat[off:off + g.numel()].data_ptr(), g.numel(), _lib.PRL_DTYPE_BF16
        off += slot
    stock = [torch.zeros(g.shape, dtype=torch.float32, device=dev) for g in grads]
    lib, stream = _lib.load(), _lib.current_stream_ptr(dev)

    def torch_add():
        for a, g in zip(stock, grads):
            a.add_(g)

    calls = {"fold_add": lambda: _lib.check(lib.prl_optim_grad_accumulate(table, len(grads), 0, stream)),
             "fold_overwrite": lambda: _lib.check(lib.prl_optim_grad_accumulate(table, len(grads), 1, stream)),
             "torch_add": torch_add}
    bytes_per_element = {"fold_add": 10, "fold_overwrite": 6, "torch_add": 10}
    times = {k: [] for k in calls}
    for k in range(warmup + steps):  # interleaved: the three see the same clocks
        for name, call in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            if k >= warmup:
                times[name].append(a.elapsed_time(b))
    # the two accumulators took the same folds in another order of calls: (warmup + steps) adds each, the flat one restarted by every overwrite
    out = {"tensors": len(grads), "numel": numel, "steps": steps, "warmup": warmup, "results": {}}
    for name, t in times.items():
        med = statistics.median(t)
        gbs = numel * bytes_per_element[name] / (med * 1e-3) / 1e9
        out["results"][name] = {"median_ms": med, "min_ms": min(t), "max_ms": max(t), "bytes_per_element": bytes_per_element[name],
                                "algorithmic_bytes": numel * bytes_per_element[name], "achieved_gbs": gbs, "frac_of_peak": gbs / PEAK_GBS,
                                "frac_of_copy_ceiling": gbs / COPY_CEILING_GBS}
    return out


def run_adafactor(steps: int, warmup: int, max_norm: float) -> dict:
    import torch
    from transformers.optimization import Adafactor

    from pipelinerl_amd.finetune.optim import FusedAdafactor
    from pipelinerl_amd.weight_sync_probe import qwen25_shapes

    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    sets = ([], [])
    for name, shape in qwen25_shapes("0p5b"):
        dtype = torch.float32 if name == "lm_head.weight" else torch.bfloat16
        w = torch.empty(shape, dtype=dtype, device=dev).normal_(0.0, 0.02, generator=gen)
        g = torch.empty(shape, dtype=dtype, device=dev).normal_(0.0, 1e-3, generator=gen)
        for params in sets:
            p = torch.nn.Parameter(w.clone())
            p.grad = g.clone()
            params.append(p)
    fused = FusedAdafactor(sets[0], lr=1e-6, master_weights=True)
    stock = Adafactor(sets[1], lr=1e-6, relative_step=False, scale_parameter=False)

    calls = {"fused_adafactor": lambda: fused.clip_and_step(max_norm), "transformers": None}
    times = {k: [] for k in calls}
    for k in range(warmup + steps):  # alternating: the two see the same clocks
        for name in calls:
            if name == "transformers":
                saved = [p.grad.clone() for p in sets[1]]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            if name == "transformers":
                torch.nn.utils.clip_grad_norm_(sets[1], max_norm)
                stock.step()
            else:
                calls[name]()
            b.record()
            b.synchronize()
            if name == "transformers":  # clip_grad_norm_ rescaled the gradients in place: put them back, outside the timed window
                for p, g in zip(sets[1], saved):
                    p.grad = g
            if k >= warmup:
                times[name].append(a.elapsed_time(b))
    alg = 0
    for p in sets[0]:
        e = p.element_size()
        alg += p.numel() * (e + 3 * e + (4 + 4 + 2 if e == 2 else 4 + 4))  # norm; three reads of the gradient; weights read and written (+ the bf16 image)
    out = {"tensors": len(sets[0]), "numel": sum(p.numel() for p in sets[0]), "steps": steps, "warmup": warmup, "max_norm": max_norm, "results": {}}
    for name, t in times.items():
        out["results"][name] = {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)}
    r = out["results"]["fused_adafactor"]
    gbs = alg / (r["median_ms"] * 1e-3) / 1e9
    r.update(algorithmic_bytes=alg, achieved_gbs=gbs, frac_of_peak=gbs / PEAK_GBS, frac_of_copy_ceiling=gbs / COPY_CEILING_GBS)
    return out


COMPACT_CONFIGS = {
    "fp32_state": dict(master_weights=False),
    "fp32_state_master": dict(master_weights=True),
    "compact": dict(master_weights=False, state_dtype="bf16", param_rounding="stochastic"),
}


def compact_step_bytes(p, kw) -> int:
    """Algorithmic bytes of one AdamW step of one parameter: g, weights, m, v read; weights (+ the bf16 image under a master), m, v written."""
    e, s = p.element_size(), (2 if kw.get("state_dtype") == "bf16" else 4)
    master = kw["master_weights"] and e == 2
    return p.numel() * (e + (4 if master else e) + 2 * s + (4 if master else 0) + e + 2 * s)


def run_compact(steps: int, warmup: int) -> dict:
    import torch

    from pipelinerl_amd.finetune.optim import FusedAdamW
    from pipelinerl_amd.weight_sync_probe import qwen25_shapes

    dev = torch.device("cuda", 0)
    shapes = qwen25_shapes("7b")
    full = len(shapes)
    free, _ = torch.cuda.mem_get_info(dev)

    def need(shapes):  # parameters and gradients once, the state of every configuration (8 + 12 + 4 B per bf16 element)
        total = 0
        for name, shape in shapes:
            n = 1
            for d in shape:
                n *= d
            e = 4 if name == "lm_head.weight" else 2
            total += n * (2 * e + 8 + (12 if e == 2 else 8) + 4)
        return total

    while need(shapes) > 0.85 * free:  # the largest prefix of the list that fits
        shapes = shapes[:-1]
    params = []
    gen = torch.Generator(device=dev).manual_seed(0)
    for name, shape in shapes:
        dtype = torch.float32 if name == "lm_head.weight" else torch.bfloat16
        p = torch.nn.Parameter(torch.empty(shape, dtype=dtype, device=dev).normal_(0.0, 0.02, generator=gen))
        p.grad = torch.empty(shape, dtype=dtype, device=dev).normal_(0.0, 1e-3, generator=gen)
        params.append(p)
    opts = {}
    for name, kw in COMPACT_CONFIGS.items():
        kw = dict(kw)
        if kw.get("state_dtype") == "bf16":
            kw["state_dtype"] = torch.bfloat16
        opts[name] = FusedAdamW(params, lr=1e-6, **kw)
    times = {k: [] for k in opts}
    for k in range(warmup + steps):  # alternating: the three see the same clocks
        for name, opt in opts.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            opt.step()
            b.record()
            b.synchronize()
            if k >= warmup:
                times[name].append(a.elapsed_time(b))
    out = {"tensors": len(params), "of_tensors": full, "numel": sum(p.numel() for p in params), "steps": steps, "warmup": warmup, "results": {}}
    for name, t in times.items():
        med = statistics.median(t)
        alg = sum(compact_step_bytes(p, COMPACT_CONFIGS[name]) for p in params)
        gbs = alg / (med * 1e-3) / 1e9
        state = sum(f.numel() * f.element_size() for f in opts[name]._flat)
        out["results"][name] = {"median_ms": med, "min_ms": min(t), "max_ms": max(t), "algorithmic_bytes": alg, "achieved_gbs": gbs,
                                "frac_of_peak": gbs / PEAK_GBS, "frac_of_copy_ceiling": gbs / COPY_CEILING_GBS, "state_bytes": state}
    return out


def main_compact(args) -> None:
    cmd = [sys.executable, __file__, "--one", "compact", "--steps", str(args.steps), "--warmup", str(args.warmup)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    line = next((l for l in res.stdout.splitlines() if l.startswith("RESULT ")), None)
    if res.returncode != 0 or line is None:
        raise SystemExit(f"compact: exit status {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}")
    report = json.loads(line[len("RESULT "):])
    r = report["results"]
    spread = r["fp32_state"]["max_ms"] - r["fp32_state"]["min_ms"]
    report = {"workload": "Qwen2.5-7B parameter list, bf16 parameters and gradients, fp32 lm_head: the AdamW step alone", **report,
              "spread_fp32_state_ms": spread, "compact_gain_ms": r["fp32_state"]["median_ms"] - r["compact"]["median_ms"],
              "compact_is_not_slower_than_fp32_state": r["compact"]["median_ms"] <= r["fp32_state"]["median_ms"] + spread}
    text = json.dumps(report, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


def main_adafactor(args) -> None:
    cmd = [sys.executable, __file__, "--one", "adafactor", "--steps", str(args.steps), "--warmup", str(args.warmup), "--max-norm", str(args.max_norm)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    line = next((l for l in res.stdout.splitlines() if l.startswith("RESULT ")), None)
    if res.returncode != 0 or line is None:
        raise SystemExit(f"adafactor: exit status {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}")
    report = json.loads(line[len("RESULT "):])
    r = report["results"]
    report = {"workload": "Qwen2.5-0.5B parameter list (tied embeddings: no separate head), bf16 parameters and gradients, Adafactor, clip at %g" % args.max_norm, **report,
              "spread_transformers_ms": r["transformers"]["max_ms"] - r["transformers"]["min_ms"],
              "gain_ms": r["transformers"]["median_ms"] - r["fused_adafactor"]["median_ms"]}
    text = json.dumps(report, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


def main_grad_accum(args) -> None:
    cmd = [sys.executable, __file__, "--one", "grad_accum", "--steps", str(args.steps), "--warmup", str(args.warmup)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    line = next((l for l in res.stdout.splitlines() if l.startswith("RESULT ")), None)
    if res.returncode != 0 or line is None:
        raise SystemExit(f"grad_accum: exit status {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}")
    report = json.loads(line[len("RESULT "):])
    r = report["results"]
    spread = r["torch_add"]["max_ms"] - r["torch_add"]["min_ms"]
    gain = r["torch_add"]["median_ms"] - r["fold_add"]["median_ms"]
    report = {"workload": "Qwen2.5-7B parameter list without the fp32 lm_head: bf16 gradients folded into fp32 accumulators", **report,
              "spread_torch_add_ms": spread, "fold_add_gain_ms": gain, "fold_is_faster_by_more_than_the_spread": gain > spread}
    text = json.dumps(report, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-norm", type=float, default=0.3)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per configuration")
    ap.add_argument("--out", default=None)
    ap.add_argument("--mode", choices=("boundary", "grad_accum", "adafactor", "compact"), default="boundary",
                    help="what to time: the AdamW step boundary, the fp32 gradient fold, the Adafactor boundary, or the compact-state step")
    ap.add_argument("--one", choices=CONFIGS + ("grad_accum", "adafactor", "compact"), default=None, help="(child) run one configuration in this process")
    args = ap.parse_args()
    if args.one == "compact":
        print("RESULT " + json.dumps(run_compact(args.steps, args.warmup)), flush=True)
        return
    if args.mode == "compact":
        main_compact(args)
        return
    if args.one == "grad_accum":
        print("RESULT " + json.dumps(run_grad_accum(args.steps, args.warmup)), flush=True)
        return
    if args.mode == "grad_accum":
        main_grad_accum(args)
        return
    if args.one == "adafactor":
        print("RESULT " + json.dumps(run_adafactor(args.steps, args.warmup, args.max_norm)), flush=True)
        return
    if args.mode == "adafactor":
        main_adafactor(args)
        return
    if args.one:
        print("RESULT " + json.dumps(run_one(args.one, args.steps, args.warmup, args.max_norm)), flush=True)
        return
    results = {}
    for config in CONFIGS:
        cmd = [sys.executable, __file__, "--one", config, "--steps", str(args.steps), "--warmup", str(args.warmup), "--max-norm", str(args.max_norm)]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        line = next((l for l in res.stdout.splitlines() if l.startswith("RESULT ")), None)
        if res.returncode != 0 or line is None:
            raise SystemExit(f"{config}: exit status {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}")
        results[config] = json.loads(line[len("RESULT "):])
    a, b = results["torch"], results["fused"]
    report = {"workload": "Qwen2.5-7B parameter list, bf16 parameters and gradients, fp32 lm_head, AdamW, clip at %g" % args.max_norm,
              "results": results, "spread_torch_ms": a["max_ms"] - a["min_ms"],
              "like_for_like_gain_ms": a["median_ms"] - b["median_ms"],
              "fused_is_faster_by_more_than_the_spread": (a["median_ms"] - b["median_ms"]) > (a["max_ms"] - a["min_ms"])}
    text = json.dumps(report, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
