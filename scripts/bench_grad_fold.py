"""Time what one micro-batch costs a learner rank with sharded gradients (`FusedAdamW(shard_grads=True)`), the collective left out:
the Qwen2.5-7B parameter list (`weight_sync_probe.qwen25_shapes("7b")`: bf16 gradients, the output head's in fp32), `world = 4`, this
process standing in for rank 0.  For `exchange_bucket_bytes` of 16, 64 and 256 MiB:

  sequence_fused      per bucket: `pack_grad_bucket(k)` (prl_bucket_gather of every destination's pieces) + `fold_grad_bucket(k, recv)`
                      (ONE prl_optim_grad_accumulate_ranks over the own pieces) - the optimizer's own methods, host work included
  sequence_separate   per bucket: the same gather + `world` calls of the existing prl_optim_grad_accumulate on the same bytes
  folds_fused         the folds alone, tables built beforehand            (8 + world x itemsize bytes per own element)
  folds_separate      the `world` separate folds alone, tables built beforehand   (world x (8 + itemsize) bytes per own element)

The four alternate inside one loop after warm-up, device events around each, `--steps` repetitions (median [min, max]; the spread is
max - min).  Algorithmic bytes: a gather reads and writes every gradient byte of this rank once; a fold reads the accumulator and the
`world` copies and writes the accumulator.  Needs a GPU and fails without one.  One JSON object on stdout and in --out.

    python scripts/bench_grad_fold.py --out profiles/grad_fold_bench.json
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

PEAK_GBS = 8000.0
WORLD = 4
BUCKET_MIB = (16, 64, 256)


def run(bucket_bytes: int, params, grads, steps: int, warmup: int) -> dict:
    import torch

    from pipelinerl_amd import _lib
    from pipelinerl_amd.finetune.optim import _DTYPES, FusedAdamW

    dev = params[0].device
    opt = FusedAdamW(params, lr=1e-6, shard=(0, WORLD), grad_accum_dtype=torch.float32, shard_grads=True, exchange_bucket_bytes=bucket_bytes)
    gx = opt._exchange()
    opt._ensure_accumulators()
    n, slot, recv, mine = gx["n"], gx["slot"], gx["recv"], [per[0] for per in gx["grad"]]
    recv.view(torch.bfloat16).normal_(0.0, 1e-3)  # what the other ranks would have sent: finite values in either dtype
    _, plist, offsets, shard_len, _ = opt._layout()
    index = {id(p): i for i, p in enumerate(plist)}
    lib, stream = _lib.load(), _lib.current_stream_ptr(dev)

    def tables(k):
        fused = (_lib.PrlAccumRanksSegment * max(len(mine[k]), 1))()
        separate = [(_lib.PrlAccumSegment * max(len(mine[k]), 1))() for _ in range(WORLD)]
        for j, (i, b, e, at) in enumerate(mine[k]):
            acc, dt = opt._acc_flat.data_ptr() + 4 * (offsets[i] + b), _DTYPES[opt._grad_dtype(plist[i])]
            fused[j].src, fused[j].acc, fused[j].numel, fused[j].src_dtype = recv.data_ptr() + at, acc, e - b, dt
            for r, t in enumerate(separate):
                t[j].grad, t[j].acc, t[j].numel, t[j].grad_dtype = recv.data_ptr() + r * slot + at, acc, e - b, dt
        return fused, separate

    prebuilt = [tables(k) for k in range(n)]

    def give_grads():
        for p in plist:
            p.grad = grads[index[id(p)]]
        opt._acc_zeroed.clear()

    def sequence_fused():
        for k in range(n):
            opt.pack_grad_bucket(k)
            opt.fold_grad_bucket(k, recv)

    def sequence_separate():
        for k in range(n):
            opt.pack_grad_bucket(k)
            _fused, separate = tables(k)  # built per call, as fold_grad_bucket builds its table
            for t in separate:
                _lib.check(lib.prl_optim_grad_accumulate(t, len(mine[k]), 0, stream))

    def folds_fused():
        for k in range(n):
            _lib.check(lib.prl_optim_grad_accumulate_ranks(prebuilt[k][0], len(mine[k]), WORLD, slot, 0, stream))

    def folds_separate():
        for k in range(n):
            for t in prebuilt[k][1]:
                _lib.check(lib.prl_optim_grad_accumulate(t, len(mine[k]), 0, stream))

    calls = {"sequence_fused": sequence_fused, "sequence_separate": sequence_separate, "folds_fused": folds_fused, "folds_separate": folds_separate}
    give_grads()
    opt._folded = True  # every timed fold adds (overwrite = 0), so the variants move the bytes the formulas count
    opt._acc_flat.zero_()
    times = {name: [] for name in calls}
    for rep in range(warmup + steps):  # alternating: the four see the same clocks
        for name, call in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            if rep >= warmup:
                times[name].append(a.elapsed_time(b))
    gather_bytes = 2 * sum(g.numel() * g.element_size() for g in grads)
    fold_fused = sum((e - b) * (8 + WORLD * gx["g_sizes"][i]) for per in mine for i, b, e, _ in per)
    fold_separate = sum((e - b) * WORLD * (8 + gx["g_sizes"][i]) for per in mine for i, b, e, _ in per)
    alg = {"sequence_fused": gather_bytes + fold_fused, "sequence_separate": gather_bytes + fold_separate, "folds_fused": fold_fused,
           "folds_separate": fold_separate}
    out = {"exchange_bucket_bytes": bucket_bytes, "bucket_elems": gx["bucket"], "buckets": n, "slot_bytes": slot, "shard_len": shard_len,
           "buffer_bytes_each": recv.numel(), "results": {}}
    for name, t in times.items():
        med = statistics.median(t)
        gbs = alg[name] / (med * 1e-3) / 1e9
        out["results"][name] = {"median_ms": med, "min_ms": min(t), "max_ms": max(t), "spread_ms": max(t) - min(t), "algorithmic_bytes": alg[name],
                                "achieved_gbs": gbs, "frac_of_peak": gbs / PEAK_GBS}
    r = out["results"]
    for pair in ("sequence", "folds"):
        f, s = r[f"{pair}_fused"], r[f"{pair}_separate"]
        out[f"{pair}_fused_is_not_slower_beyond_the_spread"] = f["median_ms"] <= s["median_ms"] + max(f["spread_ms"], s["spread_ms"])
    for p in plist:
        p.grad = None
    del opt, prebuilt
    torch.cuda.empty_cache()
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_grad_fold: no HIP device is visible; this measurement needs a GPU")
    from pipelinerl_amd.weight_sync_probe import qwen25_shapes

    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    params, grads = [], []
    for name, shape in qwen25_shapes("7b"):
        dtype = torch.float32 if name == "lm_head.weight" else torch.bfloat16
        params.append(torch.nn.Parameter(torch.empty(shape, dtype=dtype, device=dev)))  # never read: the layout is what counts
        grads.append(torch.empty(shape, dtype=dtype, device=dev).normal_(0.0, 1e-3, generator=gen))
    report = {"workload": f"Qwen2.5-7B parameter list, bf16 gradients, fp32 lm_head; world = {WORLD}, rank 0; one micro-batch's gathers and folds, "
                          "the collective left out", "tensors": len(params), "numel": sum(p.numel() for p in params), "steps": args.steps,
              "warmup": args.warmup, "runs": [run(mib << 20, params, grads, args.steps, args.warmup) for mib in BUCKET_MIB]}
    text = json.dumps(report, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
