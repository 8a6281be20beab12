"""The partition of sharded optimizer state (`plan_shards` of pipelinerl_amd/finetune/optim.py) against a brute force that assigns
every element of the slot-padded parameter space to `index // shard_len`, and the argument checks of the sharded constructors -
everything that is checkable without a GPU."""

import pytest
import torch

from pipelinerl_amd.finetune.optim import FusedAdamW, FusedLion, get_optimizer, plan_shards, shard_layout

SLOT = 16
NUMELS = [[1], [15], [16], [17], [16, 16], [5, 16384, 16385, 3 * 16384 + 5, 0, 7]]
WORLDS = [1, 2, 3, 4, 8]


def brute_force(numels, world):
    """Per rank the (param, element) pairs it owns: parameters back to back, each padded to a slot; the padded length rounded up to
    world x shard_len with shard_len a multiple of the slot; element at padded index j belongs to rank j // shard_len."""
    padded = sum((n + SLOT - 1) // SLOT * SLOT for n in numels)
    shard_len = 0
    while shard_len * world < padded:
        shard_len += SLOT
    owners = [[] for _ in range(world)]
    j = 0
    for i, n in enumerate(numels):
        for k in range(n):
            owners[(j + k) // shard_len].append((i, k))
        j += (n + SLOT - 1) // SLOT * SLOT
    return owners, shard_len


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("numels", NUMELS, ids=lambda n: "-".join(map(str, n)))
def test_plan_matches_the_brute_force(numels, world):
    plan = plan_shards(numels, world)
    owners, shard_len = brute_force(numels, world)
    assert len(plan) == world and shard_layout(numels, world)[1] == shard_len and shard_len % SLOT == 0
    seen = [0] * len(numels)
    for r, pieces in enumerate(plan):
        got = []
        for i, b, e in pieces:
            assert 0 <= b < e <= numels[i], (r, i, b, e)
            assert b % SLOT == 0, f"rank {r}: piece of parameter {i} begins at {b}"
            got += [(i, k) for k in range(b, e)]
            seen[i] += e - b
        assert got == owners[r], f"rank {r} of {world}"
        assert len({i for i, _, _ in pieces}) == len(pieces), "a rank owns one contiguous range: at most one piece per parameter"
        assert sum(e - b for _, b, e in pieces) <= shard_len
    assert seen == list(numels), "the pieces tile every parameter exactly once"


def test_world_larger_than_the_slot_count_gives_empty_shards():
    plan = plan_shards([1], 8)
    assert plan[0] == [(0, 0, 1)] and all(pieces == [] for pieces in plan[1:])
    plan = plan_shards([17], 8)  # two slots
    assert plan[:2] == [[(0, 0, 16)], [(0, 16, 17)]] and all(pieces == [] for pieces in plan[2:])
    assert plan_shards([], 4) == [[], [], [], []] and plan_shards([0, 0], 2) == [[], []]
    with pytest.raises(ValueError, match="world"):
        plan_shards([4], 0)


def test_slot_argument():
    plan = plan_shards([10, 10], 2, slot=4)  # padded 12 + 12 = 24 -> shard_len 12
    assert plan == [[(0, 0, 10)], [(1, 0, 10)]]
    plan = plan_shards([10, 10], 4, slot=4)  # shard_len 8
    assert plan == [[(0, 0, 8)], [(0, 8, 10), (1, 0, 4)], [(1, 4, 10)], []]


@pytest.mark.parametrize("cls", [FusedAdamW, FusedLion])
def test_shard_argument_checks(cls):
    p = [torch.nn.Parameter(torch.zeros(40))]
    with pytest.raises(ValueError, match="not both"):
        cls(p, lr=1e-3, shard=(0, 2), shard_group=object())  # (refused before the group is looked at)
    for bad in ((2, 2), (5, 2), (-1, 2), (0, 0)):
        with pytest.raises(ValueError, match=r"rank -?\d+ is not in \[0, \d+\)"):
            cls(p, lr=1e-3, shard=bad)
    opt = cls(p, lr=1e-3, shard=(1, 2))
    assert opt.shard_len == 32 and opt.state_dict()["state"] == {} and opt._flat == []  # state is lazy, nothing allocated
    assert cls(p, lr=1e-3, shard=(0, 1)).shard_len is None, "a world of one is the unsharded optimizer"
    assert cls(p, lr=1e-3).shard_len is None


@pytest.mark.parametrize("cls", [FusedAdamW, FusedLion])
def test_shard_dict_of_another_world_is_refused(cls):
    p = [torch.nn.Parameter(torch.zeros(40)), torch.nn.Parameter(torch.zeros(7))]
    saved = cls(p, lr=1e-3, shard=(1, 2)).state_dict()
    meta = saved["shard"]
    assert (meta["world"], meta["rank"], meta["slot"], meta["total_slots"]) == (2, 1, 16, 4) and meta["ranges"] == {0: (32, 40), 1: (0, 7)}
    with pytest.raises(ValueError, match=r"world of 2 .*world of 4"):
        cls(p, lr=1e-3, shard=(1, 4)).load_state_dict(saved)
    with pytest.raises(ValueError, match=r"rank 1 of a world of 2 .*rank 0 of a world of 2"):
        cls(p, lr=1e-3, shard=(0, 2)).load_state_dict(saved)
    with pytest.raises(ValueError, match=r"world of 2 .*world of 1"):
        cls(p, lr=1e-3).load_state_dict(saved)
    same = cls(p, lr=3e-3, shard=(1, 2))
    same.load_state_dict(saved)  # the same world and rank: accepted, hyper-parameters restored
    assert same.param_groups[0]["lr"] == 1e-3


def test_sharded_halves_need_sharded_state():
    opt = FusedAdamW([torch.nn.Parameter(torch.zeros(40))], lr=1e-3, grad_accum_dtype=torch.float32)
    for call in (opt.prepare_reduce, opt.local_grad_sumsq):
        with pytest.raises(RuntimeError, match="sharded state"):
            call()
    sharded = FusedAdamW([torch.nn.Parameter(torch.zeros(40))], lr=1e-3, grad_accum_dtype=torch.float32, shard=(0, 2))
    with pytest.raises(RuntimeError, match="no group"):
        sharded.reduce_accumulated()
    with pytest.raises(RuntimeError, match="no group"):
        sharded.compute_grad_norm(1.0)


def test_get_optimizer_and_pipeline_spec_pass_the_option_on(tmp_path):
    from pipelinerl_amd.pipeline_run import PipelineSpec

    model = torch.nn.Linear(8, 4)
    opt = get_optimizer("adamw_torch", model, 2e-5, 0.1, shard=(1, 2))
    assert isinstance(opt, FusedAdamW) and opt._shard == (1, 2)
    assert get_optimizer("lion", model, 2e-5, 0.1, shard=(0, 3))._shard == (0, 3)
    assert get_optimizer("lion", model, 2e-5, 0.1, shard_group=None)._shard is None
    with pytest.raises(ValueError, match="fused optimizer"):
        get_optimizer("adafactor", model, 1e-4, 0.0, shard=(0, 2))
    assert PipelineSpec(exp_path=str(tmp_path)).shard_optimizer_state is False
    assert PipelineSpec(exp_path=str(tmp_path), optimizer="adamw_hip", shard_optimizer_state=True).shard_optimizer_state is True
    with pytest.raises(ValueError, match="adamw_hip"):
        PipelineSpec(exp_path=str(tmp_path), shard_optimizer_state=True)
