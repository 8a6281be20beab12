"""Sequence-parallel attention over RCCL, one GPU per rank: the worker and the checks of tests/test_gpu_attention_sp_ddp.py with
`backend="nccl"`, at P = 2 ("sp_aligned", "sp_unaligned", the two tiny models, the GSPO step) and P = 4 ("sp_four", "sp_long" at
the op level).  Skipped below that many GPUs: on a one-GPU machine nothing here runs."""

import pytest
import torch

pytestmark = pytest.mark.gpu

P_CASES = {2: ("sp_aligned", "sp_unaligned"), 4: ("sp_four", "sp_long")}


@pytest.mark.parametrize("world", [2, 4])
def test_slices_over_rccl(libprl, cuda_device, world):
    if torch.cuda.device_count() < world:
        pytest.skip(f"needs {world} GPUs (one per rank), found {torch.cuda.device_count()}")
    from test_gpu_attention_sp_ddp import run_check

    run_check(cuda_device, world=world, backend="nccl", own_gpu=True, op_cases=P_CASES[world])
