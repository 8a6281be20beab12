"""The sequence-parallel attention interface without a GPU: argument errors of the slice op and the fold, the report of
`install_fused_attention` with and without a group, a group of size 1 against no group, the learner step's refusal of an unbound
model, and the composition itself on the CPU fallback - two gloo processes, each with its `make_slices(2)` slice of a packed row
of three sequences (the second crosses the cut), on a tiny fp32 Qwen2: logits per rank and parameter gradients summed over the
ranks against an fp64 copy of the model run sequence by sequence, held to 4 x the distance of the unsliced installed model on the
whole row (the rule of tests/test_gpu_attention_model.py).  The same model installed WITHOUT the group fails that check: each
rank then attends its slice alone, which is the bug the binding fixes."""

import copy
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

from pipelinerl_amd import fused_attention as fa
from pipelinerl_amd.fused_attention import (fold_parts, install_fused_attention, require_seq_parallel_attention, uninstall_fused_attention,
                                            varlen_attention_slice)

transformers = pytest.importorskip("transformers")

V, LENGTHS, MARGIN = 64, (17, 30, 17), 4.0  # 64 tokens, the cut at 32 falls inside the second sequence


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def tiny(dtype=torch.float32):
    torch.manual_seed(0)
    cfg = transformers.Qwen2Config(vocab_size=V, hidden_size=128, intermediate_size=256, num_hidden_layers=2, max_position_embeddings=256,
                                   tie_word_embeddings=False, attn_implementation="sdpa", num_attention_heads=2, num_key_value_heads=1)
    return transformers.Qwen2ForCausalLM(cfg).to(dtype)


def packed_row():
    """(input_ids [1, T], position_ids [1, T], targets [1, T]): every token carries a target of its own, so no loss term crosses a cut."""
    g = torch.Generator().manual_seed(5)
    t = sum(LENGTHS)
    ids = torch.randint(3, V, (1, t), generator=g)
    targets = torch.randint(0, V, (1, t), generator=g)
    pos = torch.cat([torch.arange(n) for n in LENGTHS])[None]
    return ids, pos, targets


def token_loss(logits, targets):
    logits = logits[0].double() if logits.dtype == torch.float64 else logits[0].float()
    return F.cross_entropy(logits, targets[0], reduction="sum")


def grads_of(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def rel_err(got, want):
    return float((got.detach().double() - want).abs().max() / want.abs().max())


# ---- arguments -------------------------------------------------------------------------------------------------------------------
def test_slice_op_refuses_cpu_tensors_and_bad_arguments():
    q = torch.zeros(8, 2, 64, dtype=torch.bfloat16)
    k = torch.zeros(16, 1, 64, dtype=torch.bfloat16)
    table = torch.zeros(16, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        varlen_attention_slice(q, k, k, table, table, 8, 0.125)
    check = fa._check_slice
    for patch, exc, word in (
        (dict(q_offset=9), ValueError, "q_offset 9"),
        (dict(q_offset=-1), ValueError, "q_offset -1"),
        (dict(q_offset=2.0), TypeError, "int"),
        (dict(q_offset=True), TypeError, "int"),
        (dict(q=torch.zeros(8, 2, 64)), TypeError, "bf16"),
        (dict(k_all=torch.zeros(16, 1, 32, dtype=torch.bfloat16)), ValueError, "are not"),
        (dict(q=torch.zeros(17, 2, 64, dtype=torch.bfloat16), q_offset=0), ValueError, "q_offset 0"),
        (dict(seq_start=torch.zeros(8, dtype=torch.int32)), ValueError, "WHOLE gathered row"),
        (dict(seq_end=torch.zeros(16, dtype=torch.int64)), ValueError, "int32"),
    ):
        a = dict(q=q, k_all=k, v_all=k, seq_start=table, seq_end=table, q_offset=8)
        a.update(patch)
        real = fa._lib.require_device
        fa._lib.require_device = lambda *t: None  # (past the device check: the argument checks themselves need no device)
        try:
            with pytest.raises(exc, match=word):
                check(a["q"], a["k_all"], a["v_all"], a["seq_start"], a["seq_end"], a["q_offset"])
        finally:
            fa._lib.require_device = real


def test_fold_parts_on_the_cpu_is_the_rank_order_sum_rounded_once():
    parts = torch.tensor([[1.0, 2.0 ** -9, 1e8, 3.0], [2.0 ** -9, 1.0, 1.0, -3.0], [2.0 ** -9, 2.0 ** -9, -1e8, 2.0 ** -20]])
    got = fold_parts(parts)
    assert got.dtype == torch.bfloat16 and got.shape == (4,)
    want = ((parts[0] + parts[1]) + parts[2]).to(torch.bfloat16)
    assert torch.equal(got, want)
    assert got[2] == 0.0  # (1e8 + 1) - 1e8 in fp32, in rank order: not the 1 a reordered sum gives
    # one rounding: 1 + 2^-9 + 2^-9 = 1 + 2^-8 is a tie that rounds to even 1.0 in bf16 only after the fp32 sum ... rounding each
    # partial first would give exactly the same here, so take a case where it does not: 1 + 2^-8 + 2^-8 = 1 + 2^-7 is a bf16 number
    two = torch.tensor([[1.0 + 2.0 ** -8], [2.0 ** -8]])
    assert float(fold_parts(two)) == 1.0 + 2.0 ** -7 and float(two.to(torch.bfloat16).float().sum().to(torch.bfloat16)) == 1.0
    assert torch.equal(fold_parts(parts[:1]), parts[0].to(torch.bfloat16))
    for bad in (parts.to(torch.bfloat16), torch.zeros(0, 4), torch.tensor(1.0)):
        with pytest.raises(ValueError):
            fold_parts(bad)


# ---- install: the report, a group of size 1 ------------------------------------------------------------------------------------------
@pytest.fixture
def world_of_one(tmp_path):
    import torch.distributed as dist

    assert not dist.is_initialized()
    dist.init_process_group("gloo", store=dist.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    try:
        yield dist.group.WORLD
    finally:
        dist.destroy_process_group()


def test_a_group_of_one_is_no_group(world_of_one):
    ids, pos, targets = packed_row()
    plain = install_fused_attention(tiny())
    one = install_fused_attention(tiny(), seq_parallel_group=world_of_one)
    assert plain._prl_fused_attention == one._prl_fused_attention == {"previous": "sdpa", "layers": 2, "skipped": []}
    assert not any(hasattr(m, "_prl_seq_parallel_group") for m in one.modules())
    a = plain(input_ids=ids, position_ids=pos, attention_mask=torch.ones_like(ids)).logits
    b = one(input_ids=ids, position_ids=pos, attention_mask=torch.ones_like(ids)).logits
    assert torch.equal(a, b)
    assert install_fused_attention(one, seq_parallel_group=world_of_one) is one and install_fused_attention(one) is one  # again: nothing changes
    require_seq_parallel_attention(one, world_of_one)  # size 1: nothing to bind
    require_seq_parallel_attention(one, None)


# ---- two ranks over gloo ---------------------------------------------------------------------------------------------------------------
def _rank(rank, world, port, out_dir):
    import torch.distributed as dist

    from pipelinerl_amd.finetune.rl import RLConfig
    from pipelinerl_amd.finetune.types import PipelineBatchEncoding
    from pipelinerl_amd.finetune_loop import LearnerStep

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    group = dist.group.WORLD
    ids, pos, targets = packed_row()
    t = ids.shape[1]
    batch = PipelineBatchEncoding(input_ids=ids, labels=targets, position_ids=pos, attention_mask=torch.ones_like(ids), old_logprobs=torch.zeros(1, t),
                                  ref_logprobs=torch.zeros(1, t), advantages=torch.zeros(1, t), rewards=torch.zeros(1, t), group_tokens=torch.ones(1, t),
                                  num_labels=torch.ones(1, t), overflow=torch.zeros(1, t), model_version=0, is_packed=True)
    mine = batch.make_slices(world)[rank]
    report = {}

    def run(model, key):
        model.zero_grad()
        logits = model(input_ids=mine.input_ids, position_ids=mine.position_ids, attention_mask=mine.attention_mask).logits
        token_loss(logits, mine.labels).backward()
        report[key] = {"logits": logits.detach(), "grads": grads_of(model)}

    unbound = install_fused_attention(tiny())
    run(unbound, "unbound")
    refused = None
    try:  # a learner step given the group and a model that is not bound to it raises
        LearnerStep(unbound, torch.optim.SGD(unbound.parameters(), lr=0.0), RLConfig(), train_batch_size=1, gradient_accumulation_passes=2,
                    max_train_steps=1, seq_parallel=world, seq_parallel_group=group, send_weight_updates=False)
    except RuntimeError as e:
        refused = str(e)
    report["refused"] = refused
    again = None
    try:  # ... and an installed model is not re-bound silently
        install_fused_attention(unbound, seq_parallel_group=group)
    except ValueError as e:
        again = str(e)
    report["rebind"] = again

    bound = install_fused_attention(tiny(), seq_parallel_group=group)
    report["report"] = dict(bound._prl_fused_attention)
    require_seq_parallel_attention(bound, group)
    LearnerStep(bound, torch.optim.SGD(bound.parameters(), lr=0.0), RLConfig(), train_batch_size=1, gradient_accumulation_passes=2, max_train_steps=1,
                seq_parallel=world, seq_parallel_group=group, send_weight_updates=False)
    run(bound, "bound")

    unequal = None
    try:  # slices of unequal length: every rank raises (the lengths are gathered before anything else)
        n = mine.input_ids.shape[1] - rank
        bound(input_ids=mine.input_ids[:, :n], position_ids=mine.position_ids[:, :n], attention_mask=mine.attention_mask[:, :n])
    except ValueError as e:
        unequal = str(e)
    report["unequal"] = unequal

    uninstall_fused_attention(bound)
    report["dropped"] = not any(hasattr(m, "_prl_seq_parallel_group") for m in bound.modules()) and getattr(bound, "_prl_fused_attention", None) is None
    torch.save(report, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_on_slices_of_a_packed_row(tmp_path):
    world = 2
    ids, pos, targets = packed_row()
    t = ids.shape[1]
    cut = t // world
    assert LENGTHS[0] < cut < LENGTHS[0] + LENGTHS[1]  # the second sequence crosses the cut

    # fp64, sequence by sequence
    wit = copy.deepcopy(tiny()).double()
    want_logits, at = [], 0
    for n in LENGTHS:
        sl = slice(at, at + n)
        logits = wit(input_ids=ids[:, sl], attention_mask=torch.ones(1, n, dtype=torch.long)).logits
        token_loss(logits, targets[:, sl]).backward()
        want_logits.append(logits.detach())
        at += n
    want_logits = torch.cat(want_logits, dim=1)
    want = grads_of(wit)

    # the unsliced installed model on the whole row: the yardstick
    whole = install_fused_attention(tiny())
    logits_w = whole(input_ids=ids, position_ids=pos, attention_mask=torch.ones_like(ids)).logits
    token_loss(logits_w, targets).backward()
    grads_w = grads_of(whole)

    mp.spawn(_rank, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    ranks = [torch.load(tmp_path / f"rank{r}.pt") for r in range(world)]

    for r in ranks:
        assert r["report"] == {"previous": "sdpa", "layers": 2, "skipped": [], "seq_parallel": 2}
        assert r["refused"] is not None and "not bound to the sequence-parallel group" in r["refused"]
        assert r["rebind"] is not None and "uninstall_fused_attention" in r["rebind"]
        assert r["unequal"] is not None and "equal length" in r["unequal"]
        assert r["dropped"]

    def distances(key):
        out = {}
        for rank, r in enumerate(ranks):
            sl = slice(rank * cut, (rank + 1) * cut)
            out[f"logits of rank {rank}"] = (rel_err(r[key]["logits"], want_logits[:, sl]), rel_err(logits_w[:, sl], want_logits[:, sl]))
        for name, w in want.items():
            summed = ranks[0][key]["grads"][name].double() + ranks[1][key]["grads"][name].double()
            out[name] = (rel_err(summed, w), rel_err(grads_w[name], w))
        return out

    failed = []
    for name, (sliced, unsliced) in distances("bound").items():
        print(f"[attention sp api] {name}: two ranks {sliced:.3e}  whole row {unsliced:.3e}")
        if not sliced <= MARGIN * unsliced:
            failed.append(f"{name}: two ranks {sliced:.3e} > {MARGIN:g} x whole row {unsliced:.3e}")
    assert not failed, "; ".join(failed)

    # without the binding the second rank's tokens of the crossing sequence never see its keys on the first rank
    alone = distances("unbound")
    missed = [name for name, (sliced, unsliced) in alone.items() if not sliced <= MARGIN * unsliced]
    print(f"[attention sp api] unbound: rank 1 logits {alone['logits of rank 1'][0]:.3e} from fp64; {len(missed)} of {len(alone)} tensors miss")
    assert "logits of rank 1" in missed and len(missed) > len(alone) // 2
    first, _ = alone["logits of rank 0"]
    assert first <= MARGIN * distances("bound")["logits of rank 0"][1]  # (rank 0 needs no key of rank 1: it is right either way)
