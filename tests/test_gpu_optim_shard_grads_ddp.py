"""Sharded fp32 gradient accumulators with real collectives: two processes share cuda:0, form a gloo group and each drive
`FusedAdamW(shard_group=WORLD, grad_accum_dtype=torch.float32, shard_grads=True)` over the parameter list of
tests/test_gpu_optim_sharded.py for two optimizer steps of two micro-batches through the boundary methods as the learner steps call
them: `accumulate_grads()` after every backward (here a collective: `all_to_all_single` per bucket), `reduce_accumulated()`,
`clip_and_step()` (one fp64 `all_reduce` for the norm, the bucketed `all_gather` of the weights).  One parameter has no gradient on
rank 1 in the first micro-batch of a step.

Checked: both ranks end with identical parameters and norms, bit-equal to the one-process stand-in run of the same data
(tests/test_gpu_optim_shard_grads.py, which is held to the numpy emulation and the per-entry acceptance there); the accumulator is the
own range only and no whole-model exchange buffer exists."""

from __future__ import annotations

import functools
import multiprocessing as mp
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WORLD, STEPS, MICRO = 2, 2, 2
BUCKET_BYTES = 40000  # several buckets, an edge inside a parameter
MAX_NORM = 0.05       # below every norm: the clip is engaged


@functools.lru_cache(maxsize=None)
def _grads():
    """grads[step][micro][rank][i]: numpy fp32 holding the values the device sees, or None."""
    import torch

    from optim_checks import log_uniform_grads
    from test_gpu_optim_sharded import FROZEN, NOGRAD, NUMELS, _dtype

    rng = np.random.default_rng(31337)

    def present(i, m, r):
        return i not in (FROZEN, NOGRAD) and not (i == 3 and m == 0 and r == 1)

    return [[[[torch.from_numpy(log_uniform_grads(rng, n, 1)[0]).to(_dtype(i)).float().numpy() if present(i, m, r) else None
               for i, n in enumerate(NUMELS)] for r in range(WORLD)] for m in range(MICRO)] for s in range(STEPS)]


def _worker(rank: int, world: int, port: int, out_q, backend: str = "gloo", own_gpu: bool = False) -> None:
    """`backend` "gloo" + one shared GPU (this file) or "nccl" + one GPU per rank (tests/test_gpu_multi_optim_shard_grads.py)."""
    try:
        import torch
        import torch.distributed as dist

        from pipelinerl_amd.finetune.optim import FusedAdamW
        from test_gpu_optim_sharded import _dev, _groups, _params

        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dev = torch.device("cuda", rank if own_gpu else 0)
        torch.cuda.set_device(dev)
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        params = _params(dev)
        opt = FusedAdamW(_groups(params), lr=1e-3, grad_accum_dtype=torch.float32, shard_group=dist.group.WORLD, shard_grads=True,
                         exchange_bucket_bytes=BUCKET_BYTES)
        norms = []
        for per_micro in _grads():
            for per_rank in per_micro:
                for i, (p, g) in enumerate(zip(params, per_rank[rank])):
                    p.grad = None if g is None else _dev(g, i, dev)
                opt.accumulate_grads()
                assert all(p.grad is None for p in params)
            opt.reduce_accumulated()
            norms.append(float(opt.clip_and_step(MAX_NORM)))
            assert float(opt._record[1]) < 1.0
            opt.zero_grad()
        torch.cuda.synchronize(dev)
        report = {
            "params": [p.detach().float().cpu().numpy() for p in params],  # (bf16 widens exactly) numpy: tensors would travel as fds of a dying process
            "norms": norms,
            "acc_bytes": opt._acc_flat.numel() * 4,
            "shard_len": opt.shard_len,
            "buckets": opt.n_grad_buckets(),
            "buffer_bytes": [opt._gx["send"].numel(), opt._gx["recv"].numel()],
            "whole_buffers": opt._pub is not None,
        }
        dist.barrier()
        dist.destroy_process_group()
        out_q.put((rank, report))
    except Exception as e:  # noqa: BLE001
        import traceback

        out_q.put((rank, {"exception": f"{type(e).__name__}: {e}\n{traceback.format_exc()}"}))


def test_sharded_gradients_two_ranks_over_gloo(libprl, cuda_device):
    run_two_rank_check(cuda_device, backend="gloo", own_gpu=False)


def run_two_rank_check(cuda_device, backend: str, own_gpu: bool):
    import socket

    from test_gpu_optim_shard_grads import ShardedGrads

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    procs = [ctx.Process(target=_worker, args=(r, WORLD, port, q, backend, own_gpu), daemon=True) for r in range(WORLD)]
    for p in procs:
        p.start()
    try:
        results = dict(q.get(timeout=420) for _ in range(WORLD))
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    for r in range(WORLD):
        assert "exception" not in results[r], results[r]["exception"]

    # the same data through the stand-ins of one process
    stand_in = ShardedGrads("adamw", cuda_device, WORLD, BUCKET_BYTES)
    for per_micro in _grads():
        for per_rank in per_micro:
            stand_in.fold(per_rank)
        stand_in.boundary("engaged")
    want = [p.detach().float().cpu().numpy() for p in stand_in.copies[0]]
    want_norms = [float(rec[0]) for rec in stand_in.records]
    a, b = results[0], results[1]
    for i, (pa, pb, w) in enumerate(zip(a["params"], b["params"], want)):
        assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32)), f"parameter {i}: the ranks stayed in lock-step"
        assert np.array_equal(pa.view(np.uint32), w.view(np.uint32)), f"parameter {i}: bit-equal to the stand-in run"
        assert np.all(np.isfinite(pa))
    from test_gpu_optim_sharded import _data

    assert not np.array_equal(a["params"][1], _data()[0][1]), "the steps moved the weights"
    assert a["norms"] == b["norms"] == want_norms and all(n > MAX_NORM for n in want_norms)
    for r in (a, b):
        assert r["acc_bytes"] == r["shard_len"] * 4 == stand_in.opts[0].shard_len * 4
        assert r["buckets"] == stand_in.opts[0].n_grad_buckets() > 1
        assert r["buffer_bytes"][0] == r["buffer_bytes"][1] <= WORLD * BUCKET_BYTES and not r["whole_buffers"]
