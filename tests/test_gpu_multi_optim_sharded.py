"""Sharded optimizer state over RCCL, one GPU per rank: the worker of tests/test_gpu_optim_sharded_ddp.py with `backend="nccl"`,
which takes the `reduce_scatter_tensor` (in place) and `all_gather_into_tensor` branches that gloo does not have.

Skipped where fewer than two GPUs are visible.  Nobody has run anything on two GPUs for this project: the first node with several
devices is the first time these two collectives carry the optimizer's buffers (see tests/test_gpu_multi.py for the same caveat
about every other multi-GPU path)."""

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs at least 2 GPUs")]


def test_sharded_state_under_ddp_over_rccl(libprl, cuda_device):
    from test_gpu_optim_sharded_ddp import run_two_rank_check

    run_two_rank_check(backend="nccl", own_gpu=True)
