"""Host side of the sharded fp32 gradient accumulators (ZeRO-2): the option rules of `finetune/optim.py` / `PipelineSpec`, the
argument validation of `prl_optim_grad_accumulate_ranks` (the C entry validates before any device work) with the ctypes mirror of its
segment, and the bucket plan (`bucket_elems`, `plan_buckets`) in plain Python - everything that is checkable without a GPU."""

import ctypes
import re
from pathlib import Path

import pytest
import torch

from pipelinerl_amd import _lib
from pipelinerl_amd.finetune.optim import FusedAdafactor, FusedAdamW, FusedLion, bucket_elems, get_optimizer, plan_buckets, plan_shards, shard_layout

FAKE = 0x10000  # validation never dereferences a pointer

# the parameter list of tests/test_gpu_optim_sharded.py, in its param_groups order, with its dtypes
NUMELS = [5, 16384, 16385, 3 * 16384 + 5, 0, 7, 1, 15, 16, 17, 16, 16]
BF16 = {0, 2, 3, 6, 8, 10}
ORDER = list(range(0, len(NUMELS), 2)) + list(range(1, len(NUMELS), 2))
LIST = [NUMELS[i] for i in ORDER]
ITEMSIZES = [2 if i in BF16 else 4 for i in ORDER]


def _err(libprl):
    return libprl.prl_last_error().decode()


def _table(n, numel=100, dtype=_lib.PRL_DTYPE_BF16):
    t = (_lib.PrlAccumRanksSegment * n)()
    for s in t:
        s.src, s.acc, s.numel, s.src_dtype, s.reserved = FAKE, FAKE, numel, dtype, 0
    return t


# ---- 1. options ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [FusedAdamW, FusedLion])
def test_shard_grads_option_rules(cls):
    p = [torch.nn.Parameter(torch.zeros(40))]
    plain = cls(p, lr=1e-3)
    assert plain.shard_grads is False and plain.exchange_bucket_bytes == 64 << 20
    on = cls(p, lr=1e-3, shard=(1, 2), grad_accum_dtype=torch.float32, shard_grads=True, exchange_bucket_bytes=4096)
    assert on.shard_grads is True and on.exchange_bucket_bytes == 4096 and on._acc_flat is None  # buffers are lazy
    with pytest.raises(ValueError, match="grad_accum_dtype"):
        cls(p, lr=1e-3, shard=(0, 2), shard_grads=True)
    with pytest.raises(ValueError, match="sharded state"):
        cls(p, lr=1e-3, grad_accum_dtype=torch.float32, shard_grads=True)
    for bad in (63, 0, -1, 64.0, True):
        with pytest.raises(ValueError, match="exchange_bucket_bytes"):
            cls(p, lr=1e-3, exchange_bucket_bytes=bad)
    assert cls(p, lr=1e-3, exchange_bucket_bytes=64).exchange_bucket_bytes == 64
    # a world of one is today's unsharded behaviour
    one = cls(p, lr=1e-3, shard=(0, 1), grad_accum_dtype=torch.float32, shard_grads=True)
    assert one.shard_grads is False and one._shard is None
    # the whole-buffer halves belong to the other mode and say where to go; the new halves belong to this one
    for call in (on.prepare_reduce, on.finish_reduce):
        with pytest.raises(RuntimeError, match="pack_grad_bucket"):
            call()
    for call in (on.pack_shard, lambda: on.unpack_shards(torch.zeros(1, dtype=torch.uint8))):
        with pytest.raises(RuntimeError, match="pack_shard_bucket"):
            call()
    other = cls(p, lr=1e-3, shard=(1, 2), grad_accum_dtype=torch.float32)
    for call in (other.n_grad_buckets, lambda: other.pack_grad_bucket(0), lambda: other.fold_grad_bucket(0, None), other.finish_grad_fold,
                 lambda: other.pack_shard_bucket(0), lambda: other.unpack_shard_bucket(0, None)):
        with pytest.raises(RuntimeError, match="shard_grads=True"):
            call()
    with pytest.raises(RuntimeError, match="no group"):
        on.accumulate_grads()  # a collective: shard= has nobody to call


def test_adafactor_and_get_optimizer_rules():
    p = [torch.nn.Parameter(torch.zeros(4, 4))]
    with pytest.raises(ValueError, match="shard_grads"):
        FusedAdafactor(p, lr=1e-3, grad_accum_dtype=torch.float32, shard_grads=True)
    model = torch.nn.Linear(4, 4)
    for name, cls in (("adamw_torch", FusedAdamW), ("lion", FusedLion)):
        opt = get_optimizer(name, model, 2e-5, 0.1, grad_accum_dtype=torch.float32, shard=(0, 2), shard_grads=True, exchange_bucket_bytes=1 << 20)
        assert isinstance(opt, cls) and opt.shard_grads and opt.exchange_bucket_bytes == 1 << 20
        assert get_optimizer(name, model, 2e-5, 0.1).shard_grads is False
        with pytest.raises(ValueError, match="grad_accum_dtype"):
            get_optimizer(name, model, 2e-5, 0.1, shard=(0, 2), shard_grads=True)
    for name in ("adafactor_hip", "adafactor"):
        with pytest.raises(ValueError, match='"adamw_torch" or "lion"'):
            get_optimizer(name, model, 1e-4, 0.0, shard_grads=True)
        with pytest.raises(ValueError, match='"adamw_torch" or "lion"'):
            get_optimizer(name, model, 1e-4, 0.0, exchange_bucket_bytes=1 << 20)


def test_pipeline_spec_shard_grad_accumulators(tmp_path):
    from pipelinerl_amd.pipeline_run import PipelineSpec

    assert PipelineSpec(exp_path=str(tmp_path)).shard_grad_accumulators is False
    ok = PipelineSpec(exp_path=str(tmp_path), optimizer="adamw_hip", grad_accum_fp32=True, shard_optimizer_state=True, shard_grad_accumulators=True)
    assert ok.shard_grad_accumulators is True
    for missing in (dict(grad_accum_fp32=True), dict(shard_optimizer_state=True), {}):
        with pytest.raises(ValueError, match="shard_grad_accumulators"):
            PipelineSpec(exp_path=str(tmp_path), optimizer="adamw_hip", shard_grad_accumulators=True, **missing)


# ---- 2. the C entry ------------------------------------------------------------------------------------------------------------------
def test_grad_accumulate_ranks_argument_validation(libprl):
    call = libprl.prl_optim_grad_accumulate_ranks
    cap = _lib.PRL_ACCUM_RANKS_MAX_WORLD
    for overwrite in (0, 1):
        assert call(None, -1, 2, 64, overwrite, None) == _lib.PRL_EINVAL and "negative" in _err(libprl)
        assert call(None, 2, 2, 64, overwrite, None) == _lib.PRL_EINVAL and "null segment table" in _err(libprl)
        t = _table(3)
        t[1].numel = -4
        assert call(t, 3, 2, 64, overwrite, None) == _lib.PRL_EINVAL and "segment 1" in _err(libprl) and "numel" in _err(libprl)
        t = _table(3)
        t[2].src_dtype = 7
        assert call(t, 3, 2, 64, overwrite, None) == _lib.PRL_EINVAL and "segment 2" in _err(libprl) and "src_dtype" in _err(libprl)
        t = _table(3, dtype=_lib.PRL_DTYPE_F32)
        t[1].acc = None  # a live piece without an accumulator
        assert call(t, 3, 2, 64, overwrite, None) == _lib.PRL_EINVAL and "segment 1" in _err(libprl) and "acc" in _err(libprl)
        for world in (0, -1, cap + 1):
            assert call(_table(1), 1, world, 64, overwrite, None) == _lib.PRL_EINVAL and "world" in _err(libprl)
        for stride in (-16, 8, 24, 100):
            assert call(_table(1), 1, 2, stride, overwrite, None) == _lib.PRL_EINVAL and "rank_stride_bytes" in _err(libprl)
        # nothing to do is not an error and touches no device: an empty table, and segments that are skipped
        assert call(None, 0, 1, 0, overwrite, None) == 0
        assert call(_table(1), 0, cap, 1 << 40, overwrite, None) == 0
        t = _table(2)
        t[0].src, t[0].acc = None, None
        t[1].numel, t[1].acc = 0, None
        assert call(t, 2, 4, 4096, overwrite, None) == 0


def test_accum_ranks_segment_struct_matches_the_header():
    text = (Path(__file__).resolve().parent.parent / "include" / "prl.h").read_text()
    body = re.search(r"typedef struct prl_accum_ranks_segment \{(.*?)\} prl_accum_ranks_segment;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(const void\*|void\*|int64_t|int32_t)\s+(\w+)\s*;", body)
    ctype = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}
    assert [(name, ctype[t]) for t, name in fields] == list(_lib.PrlAccumRanksSegment._fields_)
    assert [name for _, name in fields] == ["src", "acc", "numel", "src_dtype", "reserved"]
    assert ctypes.sizeof(_lib.PrlAccumRanksSegment) == 2 * 8 + 8 + 2 * 4
    assert _lib.PROTOTYPES["prl_optim_grad_accumulate_ranks"] == (
        ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p])
    assert int(re.search(r"#define PRL_ACCUM_RANKS_MAX_WORLD (\d+)", text).group(1)) == _lib.PRL_ACCUM_RANKS_MAX_WORLD
    assert _lib.PRL_ABI_VERSION == 19


# ---- 3. the bucket plan --------------------------------------------------------------------------------------------------------------
def test_bucket_elems():
    assert bucket_elems(64) == 16 and bucket_elems(127) == 16 and bucket_elems(128) == 32
    assert bucket_elems(64, widest=2) == 32 and bucket_elems(64 << 20) == 16 << 20 and bucket_elems(64 << 20, widest=2) == 32 << 20
    for limit in (64, 100, 4096, 1 << 20):
        for widest in (2, 4):
            b = bucket_elems(limit, widest)
            assert b % 16 == 0 and b >= 16 and b * widest <= limit < (b + 16) * widest
    with pytest.raises(ValueError, match="exchange_bucket_bytes"):
        bucket_elems(63)
    with pytest.raises(ValueError, match="multiple of the slot"):
        plan_buckets(LIST, ITEMSIZES, 2, 24)


@pytest.mark.parametrize("world", [2, 3, 4, 8])
@pytest.mark.parametrize("limit", [1 << 30, 40000, 4096, 64])  # one bucket; a few buckets, an edge inside a parameter; many; B = 16
def test_bucket_plan_tiles_every_rank_range_once(world, limit):
    offsets, shard_len = shard_layout(LIST, world)
    bucket = bucket_elems(limit, max(ITEMSIZES))
    n, slot, pieces = plan_buckets(LIST, ITEMSIZES, world, bucket)
    assert n == max(1, -(-shard_len // bucket)) and len(pieces) == n and all(len(per) == world for per in pieces)
    if limit == 1 << 30:
        assert n == 1
    elif limit == 64:
        assert bucket == 16 and n == shard_len // 16
    else:
        assert n > 1
    assert 16 <= slot <= limit and slot % 16 == 0, "no slot exceeds the limit"
    covered = [[0] * numel for numel in LIST]
    inside = False
    for k, per in enumerate(pieces):
        for d, dest in enumerate(per):
            lo, hi = d * shard_len + k * bucket, d * shard_len + min((k + 1) * bucket, shard_len)
            end = 0
            for i, b, e, at in dest:
                assert 0 <= b < e <= LIST[i] and lo <= offsets[i] + b and offsets[i] + e <= hi, "a piece lies in its bucket of its rank's range"
                assert b % 16 == 0, "a piece begins on a slot boundary of its parameter"
                assert at % 16 == 0 and at >= end, "16-byte aligned, no overlap"
                end = at + (e - b) * ITEMSIZES[i]
                inside |= 0 < b or e < LIST[i]
                for x in range(b, e):
                    covered[i][x] += 1
            assert end <= slot
            assert [i for i, *_ in dest] == sorted(i for i, *_ in dest), "plan order"
    assert all(c == 1 for per in covered for c in per), "every element of every parameter in exactly one piece"
    assert inside, "a bucket or rank edge falls inside a parameter"
    # the buckets of rank d together are rank d's pieces of the state partition
    for d, owned in enumerate(plan_shards(LIST, world)):
        got = sorted((i, b, e) for per in pieces for i, b, e, _ in per[d])
        merged = []
        for i, b, e in got:
            if merged and merged[-1][0] == i and merged[-1][2] == b:
                merged[-1] = (i, merged[-1][1], e)
            else:
                merged.append((i, b, e))
        assert merged == sorted(owned)
    # the same B with the other exchange's item sizes (weights: the parameter's dtype) cuts the same element ranges
    n2, slot2, pieces2 = plan_buckets(LIST, [4] * len(LIST), world, bucket)
    assert n2 == n and slot2 <= bucket * 4
    assert [[[(i, b, e) for i, b, e, _ in dest] for dest in per] for per in pieces2] == [[[(i, b, e) for i, b, e, _ in dest] for dest in per] for per in pieces]
