"""Sharded fp32 gradient accumulators (ZeRO-2, `shard_grads=True`) of `FusedAdamW` / `FusedLion` on the GPU, one process standing in
for every rank: the parameter list, the FROZEN / NOGRAD entries and the stand-in pattern of tests/test_gpu_optim_sharded.py, the
all-to-all and the all-gather done by hand with torch ops between the halves the methods are made of.

One micro-batch per step: parameters, every state tensor and the norm record are bit-equal to the existing `shard=(r, W)` fp32 mode
on the same data, run side by side - that stand-in adds the ranks' accumulators in rank order, which is the order of the fused fold -
and through tests/test_gpu_optim_sharded.py that ties the new mode to the unsharded run.  Three micro-batches per step, one parameter
receiving a gradient only on some ranks in some micro-batches: every owned accumulator is bit-equal to a numpy float32 emulation
(micro-batch outer, rank inner, +0.0 where nothing arrived), and the parameters pass the per-entry acceptance of tests/optim_checks.py
(fp64 witness, 4 x the fp32 CPU reference's own error), also on the entries within 16 elements of every piece edge and bucket edge held
to the whole set's r_ref.  On these inputs the fp32 CPU reference passes that bound: r_ref is its own worst entry and the edge entries
are a subset of the same set; the test asserts it."""

import functools

import numpy as np
import pytest
import torch

from optim_checks import adamw_trajectory, check_entries, lion_trajectory, log_uniform_grads
from test_gpu_optim_sharded import BF16, FROZEN, MAX_NORM, NOGRAD, NUMELS, ORDER, STEPS, WORLDS, Sharded, _cls, _data, _dev, _dtype, _groups, _lr, _params, _wd

pytestmark = pytest.mark.gpu

ONE, EDGE, MANY, B16 = 1 << 30, 40000, 4096, 64  # exchange_bucket_bytes: one bucket; a bucket edge inside a parameter; many buckets; B = 16
MICRO = 3
PARTIAL = 3  # (bf16, several chunks, cut by rank and bucket edges) receives a gradient only on some ranks in some micro-batches


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


class ShardedGrads:
    """W stand-ins with sharded gradients; the collectives by hand."""

    def __init__(self, name, device, world, bucket_bytes, **kw):
        from pipelinerl_amd.finetune.optim import plan_shards

        self.copies = [_params(device) for _ in range(world)]
        self.opts = [_cls(name)(_groups(ps), lr=_lr(name), shard=(r, world), grad_accum_dtype=torch.float32, shard_grads=True,
                                exchange_bucket_bytes=bucket_bytes, **kw) for r, ps in enumerate(self.copies)]
        self.device, self.world, self.bucket_bytes = device, world, bucket_bytes
        self.plan = [[(ORDER[k], b, e) for k, b, e in pieces] for pieces in plan_shards([NUMELS[i] for i in ORDER], world)]  # in NUMELS indices
        self.records = []

    def fold(self, grads):
        """One micro-batch: `grads[r][i]` is rank r's gradient of parameter i (numpy, the values the device sees) or None."""
        for ps, gs in zip(self.copies, grads):
            for i, (p, g) in enumerate(zip(ps, gs)):
                p.grad = None if g is None else _dev(g, i, self.device)
        n = self.opts[0].n_grad_buckets()
        assert all(o.n_grad_buckets() == n for o in self.opts)
        for k in range(n):
            sends = [o.pack_grad_bucket(k).clone() for o in self.opts]
            slot = sends[0].numel() // self.world
            assert all(s.numel() == self.world * slot and s.dtype == torch.uint8 for s in sends)
            for d, o in enumerate(self.opts):  # the all-to-all: slot r of what rank d receives is slot d of what rank r sent
                o.fold_grad_bucket(k, torch.cat([s[d * slot:(d + 1) * slot] for s in sends]))
        for o, ps in zip(self.opts, self.copies):
            o.finish_grad_fold()
            assert all(p.grad is None for p in ps), "p.grad is None after every fold"

    def boundary(self, clip):
        for o in self.opts:
            o.reduce_accumulated()  # moves nothing: no group is needed
        parts = [o.local_grad_sumsq().clone() for o in self.opts]
        tot = parts[0].clone()
        for x in parts[1:]:
            tot += x
        for o in self.opts:
            o.norm_from_sumsq(tot, MAX_NORM[clip])
        recs = [o._record.clone() for o in self.opts]
        assert all(torch.equal(_bits(recs[0]), _bits(x)) for x in recs), "norm and coefficient identical on every rank"
        self.records.append(recs[0])
        for o in self.opts:
            o.step(clipped=clip != "none")
        self.exchange_weights()
        for o in self.opts:
            o.zero_grad()

    def exchange_weights(self):
        for k in range(self.opts[0].n_grad_buckets()):
            gathered = torch.cat([o.pack_shard_bucket(k).clone() for o in self.opts])
            for o in self.opts:
                o.unpack_shard_bucket(k, gathered)

    def check_allocation(self):
        from pipelinerl_amd.finetune.optim import shard_layout

        shard_len = shard_layout([NUMELS[i] for i in ORDER], self.world)[1]
        for r, o in enumerate(self.opts):
            assert o.shard_len == shard_len and o._acc_flat.numel() * o._acc_flat.element_size() == shard_len * 4, "the own range only"
            gx = o._gx
            for buf in (gx["send"], gx["recv"]):
                assert buf.numel() == self.world * gx["slot"] <= self.world * self.bucket_bytes
            assert o._pub is None, "no whole-model exchange buffers"
            assert set(o._acc) == {self.copies[r][i] for i, _, _ in self.plan[r]} | ({self.copies[r][4]} if r == 0 else set()), "views for owned pieces only"
            for i, b, e in self.plan[r]:
                assert o._acc[self.copies[r][i]].numel() == e - b
            with pytest.raises(RuntimeError, match="pack_grad_bucket"):
                o.prepare_reduce()


def _micro_grads(s, world):
    """One micro-batch per step: the data of tests/test_gpu_optim_sharded.py, as `fold` takes it."""
    _, grads = _data()
    return [[None if i in (FROZEN, NOGRAD) else grads[s][r][i] for i in range(len(NUMELS))] for r in range(world)]


def _assert_same_run(new, old, tag):
    for r in range(new.world):
        for i, (p, q) in enumerate(zip(new.copies[r], old.copies[r])):
            assert torch.equal(_bits(p), _bits(q)), f"{tag}: parameter {i} on rank {r}"
        assert len(new.opts[r]._table_params) == len(old.opts[r]._table_params)
        for i, b, e in old.plan[r]:
            sp, sq = new.opts[r].state[new.copies[r][i]], old.opts[r].state[old.copies[r][i]]
            assert set(sp) == set(sq) and "exp_avg" in sq, (r, i)
            for k, v in sq.items():
                assert sp[k].dtype == v.dtype and sp[k].shape == v.shape and torch.equal(_bits(sp[k]), _bits(v)), f"{tag}: rank {r} {k}[{b}:{e}] of parameter {i}"
    assert len(new.records) == len(old.records)
    for s, (a, b) in enumerate(zip(new.records, old.records)):
        assert torch.equal(_bits(a), _bits(b)), f"{tag}: the norm record of step {s}: {a.tolist()} vs {b.tolist()}"


CASES = [(name, world, bb) for name in ("adamw", "lion") for world in WORLDS for bb in (ONE, EDGE)] + [("adamw", 3, B16), ("lion", 8, B16)]


@pytest.mark.parametrize("name,world,bucket_bytes", CASES)
def test_one_micro_batch_is_bit_equal_to_the_whole_buffer_sharded_run(libprl, cuda_device, name, world, bucket_bytes):
    old = Sharded(name, cuda_device, world, "fp32")
    new = ShardedGrads(name, cuda_device, world, bucket_bytes)
    n = new.opts[0].n_grad_buckets()
    assert (n == 1) if bucket_bytes == ONE else (new.opts[0]._gx["bucket"] == 16 and n == new.opts[0].shard_len // 16) if bucket_bytes == B16 else n > 1
    for s, clip in zip(range(STEPS), ("engaged", "above", "engaged")):
        old.step(s, clip)
        new.fold(_micro_grads(s, world))
        new.check_allocation()
        new.boundary(clip)
        assert float(new.records[s][1]) < 1.0 if clip == "engaged" else float(new.records[s][1]) == 1.0
    _assert_same_run(new, old, f"{name} W={world} {bucket_bytes} B")
    old.assert_every_rank_worked(STEPS)
    for r, o in enumerate(new.opts):
        assert all(float(o.state[new.copies[r][i]]["step"]) == STEPS for i, _, _ in new.plan[r])


def test_compact_state_is_bit_equal_to_the_whole_buffer_sharded_compact_run(libprl, cuda_device):
    kw = dict(state_dtype=torch.bfloat16, param_rounding="stochastic", seed=77, master_weights=False)
    old = Sharded("adamw", cuda_device, 3, "fp32", **kw)
    new = ShardedGrads("adamw", cuda_device, 3, EDGE, **kw)
    for s in range(STEPS):
        old.step(s, "engaged")
        new.fold(_micro_grads(s, 3))
        new.boundary("engaged")
    _assert_same_run(new, old, "compact adamw W=3")
    st = new.opts[0].state[new.copies[0][0]]
    assert st["exp_avg"].dtype == torch.bfloat16 and "master" not in st


# ---- three micro-batches per step ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _multi_data(world):
    """grads[step][micro][rank][i] (numpy fp32 holding the values the device sees, or None) and the numpy float32 emulation of what the
    owners accumulate: micro-batch outer, rank inner, +0.0 where a rank has nothing, the first term overwriting."""
    rng = np.random.default_rng(9000 + world)

    def present(i, s, m, r):
        if i in (FROZEN, NOGRAD):
            return False
        if i != PARTIAL:
            return True
        return m != 1 and (r + m + s) % 2 == 0  # never in micro-batch 1; on every other rank otherwise, not rank 0 in the first fold of step 1

    grads = [[[[torch.from_numpy(log_uniform_grads(rng, n, 1)[0]).to(_dtype(i)).float().numpy() if present(i, s, m, r) else None
                for i, n in enumerate(NUMELS)] for r in range(world)] for m in range(MICRO)] for s in range(STEPS)]
    sums = []
    for s in range(STEPS):
        per = []
        for i, n in enumerate(NUMELS):
            acc = None
            for m in range(MICRO):
                for r in range(world):
                    g = grads[s][m][r][i]
                    g = np.zeros(n, dtype=np.float32) if g is None else g
                    acc = g.copy() if acc is None else acc + g
            per.append(acc)
        sums.append(per)
    return grads, sums


@functools.lru_cache(maxsize=None)
def _multi_run(name, world, bucket_bytes):
    """Three steps of three micro-batches, clip engaged; checks every owned accumulator against the emulation on the way."""
    device = torch.device("cuda", 0)
    grads, sums = _multi_data(world)
    run = ShardedGrads(name, device, world, bucket_bytes)
    for s in range(STEPS):
        for m in range(MICRO):
            run.fold(grads[s][m])
        for r, o in enumerate(run.opts):
            for i, b, e in run.plan[r]:
                got, want = o._acc[run.copies[r][i]].cpu().numpy(), sums[s][i][b:e]
                bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
                assert bad.size == 0, f"step {s} rank {r}: accumulator [{b}, {e}) of parameter {i}: {bad.size} entries differ from the emulation, first at {bad[0]}"
        run.check_allocation()
        run.boundary("engaged")
        assert float(run.records[s][1]) < 1.0
    return run


def _bucket_edges(run, r, i, b, e):
    """Mask over [b, e) of parameter i: within 16 elements of a piece edge or of a bucket edge."""
    from pipelinerl_amd.finetune.optim import shard_layout

    offsets, shard_len = shard_layout([NUMELS[j] for j in ORDER], run.world)
    off = offsets[ORDER.index(i)] - r * shard_len  # the parameter's first element in this rank's range
    bucket = run.opts[r]._gx["bucket"]
    near = np.zeros(e - b, dtype=bool)
    near[:16] = True
    near[-16:] = True
    at = (off + np.arange(b, e)) % bucket
    return near | (at < 16) | (at >= bucket - 16)


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("name", ["adamw", "lion"])
def test_three_micro_batches_accumulators_and_per_entry_acceptance(libprl, cuda_device, name, world):
    run = _multi_run(name, world, EDGE)
    grads, sums = _multi_data(world)
    assert any(grads[s][0][r][PARTIAL] is None for s in range(STEPS) for r in range(world)) and any(g[PARTIAL] is not None for g in grads[0][0])
    assert run.opts[0].n_grad_buckets() > 1
    coefs = [float(rec[1]) for rec in run.records]
    p0, _ = _data()
    n_q = 3 if name == "adamw" else 2
    K, R, W, S, keep, edge = ([[] for _ in range(n_q)] for _ in range(6))
    for i, n in enumerate(NUMELS):
        if n == 0:
            continue
        g = [torch.from_numpy(sums[s][i]).to(cuda_device).div_(world).cpu().numpy() for s in range(STEPS)]  # what reduce_accumulated leaves: torch's fp32 division
        if name == "adamw":
            r32, _ = adamw_trajectory(p0[i], g, coefs, _lr(name), _wd(i), dtype=torch.float32)
            w64, scales = adamw_trajectory(p0[i], g, coefs, _lr(name), _wd(i), dtype=torch.float64)
            decided = np.ones(n, dtype=bool)
        else:
            zeros = np.zeros_like(p0[i])
            r32, _ = lion_trajectory(p0[i], zeros, g, coefs, _lr(name), _wd(i), dtype=np.float32)
            w64, scales = lion_trajectory(p0[i], zeros, g, coefs, _lr(name), _wd(i), dtype=np.float64)
            decided = np.logical_and.reduce([w[2] for w in w64] + [r[2] for r in r32])
        for r, o in enumerate(run.opts):
            be = {j: (b, e) for j, b, e in run.plan[r]}.get(i)
            if be is None:
                continue
            b, e = be
            p = run.copies[r][i]
            st = o.state[p]
            weights = st["master"] if "master" in st else p.detach().view(-1)[b:e]
            if i in BF16:
                assert torch.equal(p.detach().view(-1)[b:e], st["master"].to(torch.bfloat16)), "bf16 parameter = RNE(master)"
            got = [weights.float().cpu().numpy(), st["exp_avg"].cpu().numpy()] + ([st["exp_avg_sq"].cpu().numpy()] if name == "adamw" else [])
            near = _bucket_edges(run, r, i, b, e)
            for q in range(n_q):
                K[q].append(got[q]); R[q].append(r32[-1][q][b:e]); W[q].append(w64[-1][q][b:e]); S[q].append(scales[-1][q][b:e])
                keep[q].append(decided[b:e] if q == 0 else np.ones(e - b, dtype=bool))
                edge[q].append(near)
    for q, what in enumerate(("weights", "exp_avg", "exp_avg_sq")[:n_q]):
        k, r_, w, s_, kp, ed = (np.concatenate(x[q]) for x in (K, R, W, S, keep, edge))
        assert k.size == sum(NUMELS), "every owned piece, once"
        if name == "lion":
            assert 1.0 - kp.mean() <= 0.001, "entries whose sign is within rounding of zero"
        tag = f"shard_grads {name} W={world} {what}"
        r_ref = check_entries(tag, k, r_, w, s_, keep=kp)
        check_entries(f"{tag} (within 16 of a piece or bucket edge)", k[ed], r_[ed], w[ed], s_[ed], r_ref=r_ref, keep=kp[ed])
        # the fp32 CPU reference itself passes the bound it sets, on the whole set and on the edge subset
        check_entries(f"{tag}: the fp32 reference", r_, r_, w, s_, r_ref=r_ref, keep=kp)
        check_entries(f"{tag}: the fp32 reference (edges)", r_[ed], r_[ed], w[ed], s_[ed], r_ref=r_ref, keep=kp[ed])
    # after the exchange every rank holds the owners' parameters
    for r in range(1, world):
        for i, p in enumerate(run.copies[r]):
            assert torch.equal(_bits(p), _bits(run.copies[0][i])), f"parameter {i} differs between rank {r} and rank 0"


@pytest.mark.parametrize("name", ["adamw", "lion"])
def test_result_does_not_depend_on_the_bucket_size(libprl, cuda_device, name):
    world = 3
    runs = [_multi_run(name, world, bb) for bb in (EDGE, ONE, MANY)]
    assert [r.opts[0].n_grad_buckets() for r in runs][1] == 1 and runs[2].opts[0].n_grad_buckets() > runs[0].opts[0].n_grad_buckets() > 1
    for other in runs[1:]:
        _assert_same_run(other, runs[0], f"{name} W={world} {other.bucket_bytes} B vs {runs[0].bucket_bytes} B")


@pytest.mark.parametrize("bucket_bytes", [ONE, EDGE, MANY])
def test_bucketed_weight_exchange_equals_the_whole_buffer_exchange(libprl, cuda_device, bucket_bytes):
    """Every rank's copy of the parameters is filled with its own values; after either exchange every rank holds, piece by piece, the
    values of the piece's owner."""
    world = 4
    old = Sharded("adamw", cuda_device, world, "fp32")
    new = ShardedGrads("adamw", cuda_device, world, bucket_bytes)
    gen = torch.Generator(device="cpu").manual_seed(3)
    for r in range(world):
        for p, q in zip(new.copies[r], old.copies[r]):
            v = torch.randn(p.shape, generator=gen).to(device=cuda_device, dtype=p.dtype)
            p.data.copy_(v)
            q.data.copy_(v)
    before = [[p.detach().clone() for p in ps] for ps in new.copies]
    gathered = torch.cat([o.pack_shard().clone() for o in old.opts])
    for o in old.opts:
        o.unpack_shards(gathered)
    new.exchange_weights()
    for r in range(world):
        for i, (p, q) in enumerate(zip(new.copies[r], old.copies[r])):
            assert torch.equal(_bits(p), _bits(q)), f"rank {r} parameter {i}"
    for owner in range(world):
        for i, b, e in new.plan[owner]:
            for r in range(world):
                assert torch.equal(_bits(new.copies[r][i].view(-1)[b:e]), _bits(before[owner][i].view(-1)[b:e]))
    with pytest.raises(RuntimeError, match="pack_shard_bucket"):
        new.opts[0].pack_shard()
    assert all(o._pub is None for o in new.opts) and all(o._pub is not None for o in old.opts)


def test_set_to_none_false_and_a_micro_batch_without_gradients(libprl, cuda_device):
    """`finish_grad_fold(set_to_none=False)` zeroes in place and the zeroed gradient does not count as unfolded; it travels as +0.0."""
    world = 2
    a, b = ShardedGrads("adamw", cuda_device, world, EDGE), ShardedGrads("adamw", cuda_device, world, EDGE)
    gs = _micro_grads(0, world)
    a.fold(gs)
    a.fold([[None] * len(NUMELS)] * world)  # a micro-batch in which nobody has anything: adds +0.0
    for ps, g in zip(b.copies, gs):
        for i, (p, t) in enumerate(zip(ps, g)):
            p.grad = None if t is None else _dev(t, i, cuda_device)
    for _ in range(2):  # the second pass sees only gradients zeroed in place
        for k in range(b.opts[0].n_grad_buckets()):
            sends = [o.pack_grad_bucket(k).clone() for o in b.opts]
            slot = sends[0].numel() // world
            for d, o in enumerate(b.opts):
                o.fold_grad_bucket(k, torch.cat([s[d * slot:(d + 1) * slot] for s in sends]))
        for o, ps in zip(b.opts, b.copies):
            o.finish_grad_fold(set_to_none=False)
            assert all(p.grad is None or not p.grad.any() for p in ps) and any(p.grad is not None for p in ps)
    a.boundary("engaged")
    b.boundary("engaged")
    _assert_same_run(a, b, "set_to_none=False")
