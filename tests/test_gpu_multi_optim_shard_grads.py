"""Sharded fp32 gradient accumulators over RCCL, one GPU per rank: the worker of tests/test_gpu_optim_shard_grads_ddp.py with
`backend="nccl"`, which carries the buckets with RCCL's `all_to_all_single` and takes the `all_gather_into_tensor` branch of the
bucketed weight exchange that gloo does not have.

Skipped where fewer than two GPUs are visible.  Nobody has run anything on two GPUs for this project: the first node with several
devices is the first time these collectives carry the optimizer's buckets (see tests/test_gpu_multi.py for the same caveat about
every other multi-GPU path)."""

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs at least 2 GPUs")]


def test_sharded_gradients_two_ranks_over_rccl(libprl, cuda_device):
    from test_gpu_optim_shard_grads_ddp import run_two_rank_check

    run_two_rank_check(cuda_device, backend="nccl", own_gpu=True)
