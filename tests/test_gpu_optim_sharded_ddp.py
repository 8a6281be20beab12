"""Sharded optimizer state through the learner boundary, with real collectives: two processes share cuda:0, form a gloo group and
each run `NativeLearnerStep` under DistributedDataParallel for two optimizer steps with uneven shares (the pattern of
tests/test_gpu_native_ddp.py, whose tiny model and data this file uses) - once with
`FusedAdamW(shard_group=WORLD, grad_accum_dtype=torch.float32)` and once with the unsharded fused optimizer on an equal model.

Checked: the parameters are identical on both ranks; they are bit-equal to the unsharded run (the threshold is above the norm, so
the coefficient is exactly 1 and the per-element operations are the same); `grad_norm` is within 1 fp32 ulp of the unsharded one
(two fp64 shard sums added instead of one fixed-order fold); rank 0's `full_state_dict()` equals the unsharded state."""

from __future__ import annotations

import multiprocessing as mp
import os

import pytest

import test_gpu_native_ddp as base

pytestmark = pytest.mark.gpu

THRESHOLD = 1e6  # above every norm: the norm pass runs, the clip is not engaged


def _worker(rank: int, world: int, port: int, out_q, backend: str = "gloo", own_gpu: bool = False) -> None:
    """`backend` "gloo" + one shared GPU (this file) or "nccl" + one GPU per rank (tests/test_gpu_multi_optim_sharded.py)."""
    try:
        import torch
        import torch.distributed as dist

        from pipelinerl_amd.finetune.optim import FusedAdamW
        from pipelinerl_amd.finetune_loop import NativeLearnerStep
        from pipelinerl_amd.hotpath import dense_micro_batches

        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dev = torch.device("cuda", rank if own_gpu else 0)
        torch.cuda.set_device(dev)
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        report = {}
        for kind in ("unsharded", "sharded"):
            model = torch.nn.parallel.DistributedDataParallel(base._model(torch).to(dev), device_ids=[dev.index] if backend == "nccl" else None)
            opt = FusedAdamW(model.parameters(), lr=1e-3, grad_accum_dtype=torch.float32, shard_group=dist.group.WORLD if kind == "sharded" else None)
            native = NativeLearnerStep(model, opt, base._rl(), eos_token_id=2, samples_per_step=16, max_train_steps=20, process_group=dist.group.WORLD,
                                       gradient_clipping_threshold=THRESHOLD)
            norms = []
            for step in range(2):
                rag = base._step_data(step)
                # uneven shares of whole groups: rank 0 takes 3 groups, rank 1 one
                lo, hi = (0, 3 * base.ATTEMPTS) if rank == 0 else (3 * base.ATTEMPTS, 4 * base.ATTEMPTS)
                mine = rag.select(range(lo, hi)).to(dev)
                native.step(mine, dense_micro_batches(mine, 2 * base.SEQ))
                norms.append(native.metrics.grad_norm)
            full = opt.full_state_dict()
            report[kind] = {
                "params": [p.detach().cpu().numpy() for p in model.module.parameters()],  # numpy: tensors would travel as fds of a dying process
                "norms": norms,
                "state_bytes": sum(f.numel() * 4 for f in opt._flat),
                "owned": len(opt._table_params),
                "state": None if full is None else {pid: {k: v.cpu().numpy() for k, v in st.items()} for pid, st in full["state"].items()},
            }
        dist.barrier()
        dist.destroy_process_group()
        out_q.put((rank, report))
    except Exception as e:  # noqa: BLE001
        import traceback

        out_q.put((rank, {"exception": f"{type(e).__name__}: {e}\n{traceback.format_exc()}"}))


def test_sharded_state_under_ddp_two_ranks(libprl, cuda_device):
    run_two_rank_check(backend="gloo", own_gpu=False)


def run_two_rank_check(backend: str, own_gpu: bool):
    import socket

    import numpy as np

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, backend, own_gpu), daemon=True) for r in range(2)]
    for p in procs:
        p.start()
    try:
        results = dict(q.get(timeout=420) for _ in range(2))
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    for r in (0, 1):
        assert "exception" not in results[r], results[r]["exception"]

    a, b = results[0], results[1]
    for kind in ("unsharded", "sharded"):
        for pa, pb in zip(a[kind]["params"], b[kind]["params"]):
            assert np.array_equal(pa, pb), f"{kind}: the ranks stayed in lock-step"
        assert a[kind]["norms"] == b[kind]["norms"], f"{kind}: the same norm on both ranks"
    for ps, pu in zip(a["sharded"]["params"], a["unsharded"]["params"]):
        assert np.array_equal(ps.view(np.uint32), pu.view(np.uint32)), "clip not engaged: bit-equal to the unsharded run"
        assert np.all(np.isfinite(ps))
    assert not np.array_equal(a["sharded"]["params"][0], base._model(__import__("torch")).emb.weight.detach().numpy()), "the steps moved the weights"
    for ns, nu in zip(a["sharded"]["norms"], a["unsharded"]["norms"]):
        apart = abs(int(np.float32(ns).view(np.int32)) - int(np.float32(nu).view(np.int32)))
        print(f"[shard] grad_norm {ns!r} (sharded) vs {nu!r}: {apart} ulp")
        assert 0 < ns < THRESHOLD and apart <= 1
    # every rank owned pieces and allocated its range only: 2304 + 2304 + 96 elements -> 2 x 2352, two state keys (fp32 parameters: no master)
    for r in (a, b):
        assert r["sharded"]["owned"] >= 1 and r["sharded"]["state_bytes"] == 2352 * 4 * 2
        assert r["unsharded"]["state_bytes"] == 4704 * 4 * 2
    # the gathered state on rank 0 is the unsharded optimizer's; nothing on rank 1
    assert b["sharded"]["state"] is None and set(a["sharded"]["state"]) == set(a["unsharded"]["state"]) == {0, 1, 2}
    for pid, st in a["unsharded"]["state"].items():
        for k, v in st.items():
            got = a["sharded"]["state"][pid][k]
            assert got.shape == v.shape and np.array_equal(got, v), (pid, k)
