"""Sharded optimizer state (ZeRO-1) of `FusedAdamW` / `FusedLion` on the GPU, one process standing in for every rank: W copies of
one parameter list, each with an optimizer built with `shard=(r, W)`, the collectives done by hand with torch ops between the
halves the methods are made of, compared with ONE unsharded optimizer on the same data.

Clip not engaged: parameters and state are bit-equal to the unsharded run (the per-element operations are the same and the
coefficient is exactly 1).  The norm: the shard sums of squares added in rank order differ from the unsharded fixed-order sum in
fp64 rounding only, so the fp32 norm is equal or adjacent (<= 1 ulp); with complete gradients it is the same pass, bit for bit.
Clip engaged: the per-entry acceptance of tests/optim_checks.py (fp64 witness, 4 x the fp32 CPU reference's own error) on every
owned piece, and on the entries within 16 elements of every piece edge held to the whole set's r_ref.  On these inputs the fp32
CPU reference passes its own bound by construction (r_ref is its worst entry; the edge entries are a subset of the same set)."""

import functools

import numpy as np
import pytest
import torch

from optim_checks import adamw_trajectory, check_entries, lion_trajectory, log_uniform_grads

pytestmark = pytest.mark.gpu

# the numels of tests/test_optim_shard_plan.py in one list: sub-slot, one chunk, one chunk + 1, several chunks + a ragged tail, empty
NUMELS = [5, 16384, 16385, 3 * 16384 + 5, 0, 7, 1, 15, 16, 17, 16, 16]
BF16 = {0, 2, 3, 6, 8, 10}
FROZEN, NOGRAD = 9, 7  # (fp32 both) requires_grad=False / never receives a gradient
ORDER = list(range(0, len(NUMELS), 2)) + list(range(1, len(NUMELS), 2))  # param_groups order: the decayed group, then the other
WORLDS = [2, 3, 4, 8]
STEPS = 3
MAX_NORM = {"none": None, "above": 1e6, "engaged": 0.05}


def _cls(name):
    from pipelinerl_amd.finetune import optim

    return {"adamw": optim.FusedAdamW, "lion": optim.FusedLion}[name]


def _lr(name):
    return {"adamw": 1e-3, "lion": 1e-4}[name]


def _wd(i):
    return 0.01 if i % 2 == 0 else 0.0


def _dtype(i):
    return torch.bfloat16 if i in BF16 else torch.float32


@functools.lru_cache(maxsize=None)
def _data():
    """(p0[i], grads[step][rank][i]) as numpy fp32 holding the values the device sees (bf16 parameters: bf16-representable)."""
    rng = np.random.default_rng(4242)
    p0 = [torch.from_numpy(rng.normal(0.0, 0.05, n).astype(np.float32)).to(_dtype(i)).float().numpy() for i, n in enumerate(NUMELS)]
    grads = [[[torch.from_numpy(log_uniform_grads(rng, n, 1)[0]).to(_dtype(i)).float().numpy() for i, n in enumerate(NUMELS)]
              for _ in range(max(WORLDS))] for _ in range(STEPS + 1)]
    return p0, grads


def _params(device):
    p0, _ = _data()
    return [torch.nn.Parameter(torch.from_numpy(a).to(device=device, dtype=_dtype(i)), requires_grad=i != FROZEN) for i, a in enumerate(p0)]


def _groups(params):
    return [{"params": params[0::2], "weight_decay": _wd(0)}, {"params": params[1::2], "weight_decay": _wd(1)}]


def _dev(a, i, device, dtype=None):
    return torch.from_numpy(a).to(device=device, dtype=dtype or _dtype(i))


def _reduced_grads(step, world, mode, device):
    """What the unsharded optimizer is given.  "ddp": the complete gradient every rank holds (rank 0's draw).  "fp32": the average the
    ranks' fp32 accumulators reduce to - their sum in rank order divided by the world size, zeros where nothing was folded."""
    _, grads = _data()
    out = []
    for i in range(len(NUMELS)):
        if mode == "ddp":
            out.append(None if i in (FROZEN, NOGRAD) else _dev(grads[step][0][i], i, device))
        elif i in (FROZEN, NOGRAD):
            out.append(torch.zeros(NUMELS[i], dtype=torch.float32, device=device))
        else:
            total = _dev(grads[step][0][i], i, device).float()
            for r in range(1, world):
                total = total + _dev(grads[step][r][i], i, device).float()
            out.append(total / world)
    return out


class Unsharded:
    """One unsharded optimizer over the reduced gradients; remembers the norm record of every step."""

    def __init__(self, name, device, world, mode, clip):
        self.params = _params(device)
        self.opt = _cls(name)(_groups(self.params), lr=_lr(name))
        self.device, self.world, self.mode, self.clip = device, world, mode, clip
        self.records, self.grads = [], []

    def step(self, s):
        g = _reduced_grads(s, self.world, self.mode, self.device)
        self.grads.append([None if t is None else t.float().cpu().numpy() for t in g])
        for i, (p, t) in enumerate(zip(self.params, g)):
            if t is not None and t.dtype != p.dtype:
                p.grad_dtype = torch.float32
            p.grad = t
        self.opt.compute_grad_norm(MAX_NORM[self.clip])
        self.records.append(self.opt._record.clone())
        self.opt.step(clipped=self.clip != "none")
        self.opt.zero_grad()


class Sharded:
    """W stand-ins; `step` does the collectives by hand and checks what holds at every step whatever the clip."""

    def __init__(self, name, device, world, mode, **kw):
        from pipelinerl_amd.finetune.optim import plan_shards

        self.copies = [_params(device) for _ in range(world)]
        self.opts = [_cls(name)(_groups(ps), lr=_lr(name), shard=(r, world), grad_accum_dtype=torch.float32 if mode == "fp32" else None, **kw)
                     for r, ps in enumerate(self.copies)]
        self.device, self.world, self.mode = device, world, mode
        self.plan = [[(ORDER[k], b, e) for k, b, e in pieces] for pieces in plan_shards([NUMELS[i] for i in ORDER], world)]  # in NUMELS indices
        self.records = []

    def owned(self, r):
        return {i: (b, e) for i, b, e in self.plan[r]}

    def step(self, s, clip, expect=None):
        """`expect`: the unsharded parameters after this step - the owned elements must equal them in bits before the exchange."""
        _, grads = _data()
        for r, ps in enumerate(self.copies):
            for i, p in enumerate(ps):
                p.grad = None if i in (FROZEN, NOGRAD) else _dev(grads[s][r if self.mode == "fp32" else 0][i], i, self.device)
            if self.mode == "fp32":
                self.opts[r].accumulate_grads()
                assert all(p.grad is None for p in ps)
        if self.mode == "fp32":
            flats = [o.prepare_reduce() for o in self.opts]
            total = flats[0].clone()
            for f in flats[1:]:
                total += f
            for r, o in enumerate(self.opts):
                o.finish_reduce(total[r * o.shard_len:(r + 1) * o.shard_len])
        # the norm is formed at every step, whatever the clip: it is compared with the unsharded one
        if self.mode == "fp32":
            parts = [o.local_grad_sumsq().clone() for o in self.opts]
            tot = parts[0].clone()
            for x in parts[1:]:
                tot += x
            norms = [o.norm_from_sumsq(tot, MAX_NORM[clip]) for o in self.opts]
        else:
            norms = [o.compute_grad_norm(MAX_NORM[clip]) for o in self.opts]
        assert all(n.device.type == "cuda" and n.dim() == 0 for n in norms)
        recs = [o._record.clone() for o in self.opts]
        assert all(torch.equal(recs[0].view(torch.int32), x.view(torch.int32)) for x in recs), "norm and coefficient identical on every rank"
        self.records.append(recs[0])
        pre = [[p.detach().clone() for p in ps] for ps in self.copies]
        for o in self.opts:
            o.step(clipped=clip != "none")
        # before the exchange: only the owned elements moved
        for r, ps in enumerate(self.copies):
            mine = self.owned(r)
            for i, p in enumerate(ps):
                b, e = mine.get(i, (0, 0))
                now, was = p.detach().view(-1), pre[r][i].view(-1)
                assert torch.equal(now[:b], was[:b]) and torch.equal(now[e:], was[e:]), f"step {s} rank {r}: parameter {i} moved outside [{b}, {e})"
                if expect is not None:
                    assert torch.equal(now[b:e], expect[i].detach().view(-1)[b:e]), f"step {s} rank {r}: owned piece [{b}, {e}) of parameter {i}"
        gathered = torch.cat([o.pack_shard().clone() for o in self.opts])
        for o in self.opts:
            o.unpack_shards(gathered)
        for r, ps in enumerate(self.copies):  # after it: every rank holds the owners' values
            for i, p in enumerate(ps):
                assert torch.equal(p.detach(), self.copies[0][i].detach()), f"step {s}: parameter {i} differs between rank {r} and rank 0"
                if expect is not None:
                    assert torch.equal(p.detach(), expect[i].detach())
        for o in self.opts:
            o.zero_grad()

    def assert_every_rank_worked(self, steps):
        """No silent skip: every rank with a non-empty shard stepped at least one owned piece `steps` times."""
        for r, o in enumerate(self.opts):
            stepped = [i for i, _, _ in self.plan[r] if self.copies[r][i] in o.state and float(o.state[self.copies[r][i]]["step"]) == steps]
            assert bool(stepped) == bool([1 for i, _, _ in self.plan[r] if self.mode == "fp32" or i not in (FROZEN, NOGRAD)]), f"rank {r} of {self.world}"
            assert len(o._table_params) == len(self.plan[r]) + (r == 0), "one segment per owned piece (+ rank 0: the parameter without elements, for its step count)"
        assert all(self.plan[r] for r in range(self.world)), "this parameter list leaves no rank empty"


def _ulp_apart(a, b):
    return abs(int(a.view(torch.int32)) - int(b.view(torch.int32)))


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("clip", ["none", "above"])
@pytest.mark.parametrize("mode", ["ddp", "fp32"])
@pytest.mark.parametrize("name", ["adamw", "lion"])
def test_clip_not_engaged_is_bit_equal_to_the_unsharded_run(libprl, cuda_device, name, mode, clip, world):
    from pipelinerl_amd.finetune.optim import shard_layout

    ref = Unsharded(name, cuda_device, world, mode, clip)
    sh = Sharded(name, cuda_device, world, mode)
    keys = ("exp_avg", "exp_avg_sq") if name == "adamw" else ("exp_avg",)
    for s in range(STEPS):
        ref.step(s)
        sh.step(s, clip, expect=ref.params)
        assert float(ref.records[s][1]) == 1.0 and float(sh.records[s][1]) == 1.0
        apart = _ulp_apart(sh.records[s][0].cpu(), ref.records[s][0].cpu())
        print(f"[shard] {name} {mode} W={world} step {s}: norm {float(sh.records[s][0]):.9g}, {apart} ulp from the unsharded one")
        assert apart <= (1 if mode == "fp32" else 0)
    sh.assert_every_rank_worked(STEPS)
    for r, o in enumerate(sh.opts):
        for i, b, e in sh.plan[r]:
            p, q = sh.copies[r][i], ref.params[i]
            assert (p in o.state and len(o.state[p]) > 0) == (len(ref.opt.state[q]) > 0), (r, i)
            if not len(ref.opt.state[q]):
                continue
            st, want = o.state[p], ref.opt.state[q]
            assert float(st["step"]) == float(want["step"]) == STEPS
            for k in keys + (("master",) if i in BF16 else ()):
                assert st[k].dtype == torch.float32 and st[k].numel() == e - b
                assert torch.equal(st[k], want[k].view(-1)[b:e]), f"rank {r}: {k}[{b}:{e}] of parameter {i}"
            assert ("master" in st) == (i in BF16)
        # allocation: the own range only
        n_keys = len(keys) + 1  # + master (the list has bf16 parameters)
        assert sum(f.numel() * f.element_size() for f in o._flat) == o.shard_len * 4 * n_keys
        assert len(o._flat) == n_keys and o.shard_len == shard_layout([NUMELS[i] for i in ORDER], world)[1]
        assert sum(f.numel() * 4 for f in o._flat) < sum(f.numel() * 4 for f in ref.opt._flat), "not the full size"


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("mode", ["ddp", "fp32"])
@pytest.mark.parametrize("name", ["adamw", "lion"])
def test_clip_engaged_per_entry(libprl, cuda_device, name, mode, world):
    ref = Unsharded(name, cuda_device, world, mode, "engaged")
    sh = Sharded(name, cuda_device, world, mode)
    for s in range(STEPS):
        ref.step(s)
        sh.step(s, "engaged")
        apart = _ulp_apart(sh.records[s][0].cpu(), ref.records[s][0].cpu())
        assert apart <= (1 if mode == "fp32" else 0), (s, apart)
        assert float(sh.records[s][1]) < 1.0
    sh.assert_every_rank_worked(STEPS)
    coefs = [float(rec[1]) for rec in sh.records]
    p0, _ = _data()
    n_q = 3 if name == "adamw" else 2
    K, R, W, S, keep, edge = ([[] for _ in range(n_q)] for _ in range(6))
    for i, n in enumerate(NUMELS):
        if n == 0 or ref.grads[0][i] is None:
            continue
        g = [ref.grads[s][i] for s in range(STEPS)]
        if name == "adamw":
            r32, _ = adamw_trajectory(p0[i], g, coefs, _lr(name), _wd(i), dtype=torch.float32)
            w64, scales = adamw_trajectory(p0[i], g, coefs, _lr(name), _wd(i), dtype=torch.float64)
            decided = np.ones(n, dtype=bool)
        else:
            zeros = np.zeros_like(p0[i])
            r32, _ = lion_trajectory(p0[i], zeros, g, coefs, _lr(name), _wd(i), dtype=np.float32)
            w64, scales = lion_trajectory(p0[i], zeros, g, coefs, _lr(name), _wd(i), dtype=np.float64)
            decided = np.logical_and.reduce([w[2] for w in w64] + [r[2] for r in r32])
        for r, o in enumerate(sh.opts):
            be = sh.owned(r).get(i)
            if be is None:
                continue
            b, e = be
            p = sh.copies[r][i]
            st = o.state[p]
            weights = st["master"] if "master" in st else p.detach().view(-1)[b:e]
            if i in BF16:
                assert torch.equal(p.detach().view(-1)[b:e], st["master"].to(torch.bfloat16)), "bf16 parameter = RNE(master)"
            got = [weights.float().cpu().numpy(), st["exp_avg"].cpu().numpy()] + ([st["exp_avg_sq"].cpu().numpy()] if name == "adamw" else [])
            near = np.zeros(e - b, dtype=bool)
            near[:16] = True
            near[-16:] = True
            for q in range(n_q):
                K[q].append(got[q]); R[q].append(r32[-1][q][b:e]); W[q].append(w64[-1][q][b:e]); S[q].append(scales[-1][q][b:e])
                keep[q].append(decided[b:e] if q == 0 else np.ones(e - b, dtype=bool))
                edge[q].append(near)
    for q, what in enumerate(("weights", "exp_avg", "exp_avg_sq")[:n_q]):
        k, r_, w, s_, kp, ed = (np.concatenate(x[q]) for x in (K, R, W, S, keep, edge))
        assert k.size == sum(n for i, n in enumerate(NUMELS) if ref.grads[0][i] is not None), "every owned piece, once"
        if name == "lion":
            assert 1.0 - kp.mean() <= 0.001, "entries whose sign is within rounding of zero"
        r_ref = check_entries(f"sharded {name} {mode} W={world} {what}", k, r_, w, s_, keep=kp)
        check_entries(f"sharded {name} {mode} W={world} {what} (within 16 of a piece edge)", k[ed], r_[ed], w[ed], s_[ed], r_ref=r_ref, keep=kp[ed])


def test_norm_halves_reproduce_the_norm_record(libprl, cuda_device):
    """prl_optim_grad_sumsq + prl_optim_clip_from_sumsq on the full table = prl_optim_grad_norm's record, bit for bit."""
    from pipelinerl_amd import _lib

    ref = Unsharded("adamw", cuda_device, 1, "ddp", "engaged")
    for i, (p, t) in enumerate(zip(ref.params, _reduced_grads(0, 1, "ddp", cuda_device))):
        p.grad = t
    opt = ref.opt
    sumsq = torch.zeros(1, dtype=torch.float64, device=cuda_device)
    record = torch.zeros(2, dtype=torch.float32, device=cuda_device)
    stream = _lib.current_stream_ptr(cuda_device)
    for max_norm in (0.05, 1e6, 0.0):
        opt.compute_grad_norm(max_norm)
        want = opt._record.clone()
        table, entries = opt._current_table()
        opt._workspace.zero_()
        _lib.check(libprl.prl_optim_grad_sumsq(table, len(entries), opt._workspace.data_ptr(), opt._workspace.numel(), sumsq.data_ptr(), stream))
        _lib.check(libprl.prl_optim_clip_from_sumsq(sumsq.data_ptr(), max_norm, record.data_ptr(), stream))
        assert torch.equal(record.view(torch.int32), want.view(torch.int32)), (max_norm, record, want)
        assert float(sumsq) > 0 and abs(float(sumsq) ** 0.5 - float(want[0])) <= 2.0 ** -23 * float(want[0])
    assert (float(want[1]) == 1.0) and float(want[0]) > 0.05
    # argument checks of the new entries (before any device work)
    assert libprl.prl_optim_grad_sumsq(table, len(entries), opt._workspace.data_ptr(), opt._workspace.numel(), None, stream) == _lib.PRL_EINVAL
    assert libprl.prl_optim_grad_sumsq(table, len(entries), opt._workspace.data_ptr(), 8, sumsq.data_ptr(), stream) == _lib.PRL_EINVAL
    assert libprl.prl_optim_clip_from_sumsq(None, 1.0, record.data_ptr(), stream) == _lib.PRL_EINVAL
    assert libprl.prl_optim_clip_from_sumsq(sumsq.data_ptr(), 1.0, None, stream) == _lib.PRL_EINVAL
    # no live segment: the sum is 0
    empty = (_lib.PrlOptimSegment * 1)()
    sumsq.fill_(7.0)
    _lib.check(libprl.prl_optim_grad_sumsq(empty, 1, opt._workspace.data_ptr(), opt._workspace.numel(), sumsq.data_ptr(), stream))
    assert float(sumsq) == 0.0


@pytest.mark.parametrize("name", ["adamw", "lion"])
def test_state_round_trips_between_sharded_and_unsharded(libprl, cuda_device, name):
    """full state -> unsharded optimizer -> one more step = continuing the sharded run; unsharded state -> shards likewise."""
    from pipelinerl_amd.finetune.optim import merge_shard_state_dicts

    world, mode, clip = 3, "ddp", "above"
    ref = Unsharded(name, cuda_device, world, mode, clip)
    sh = Sharded(name, cuda_device, world, mode)
    for s in range(STEPS):
        ref.step(s)
        sh.step(s, clip, expect=ref.params)
    shard_dicts = [o.state_dict() for o in sh.opts]
    assert all(d["shard"]["world"] == world and d["shard"]["rank"] == r for r, d in enumerate(shard_dicts))
    full = merge_shard_state_dicts(shard_dicts)
    unsharded_dict = ref.opt.state_dict()
    assert set(full["state"]) == set(unsharded_dict["state"])
    for pid, st in unsharded_dict["state"].items():
        assert set(st) == set(full["state"][pid])
        for k, v in st.items():
            assert torch.equal(torch.as_tensor(v).cpu(), torch.as_tensor(full["state"][pid][k]).cpu()), (pid, k)

    # (a) the gathered dictionary in a fresh unsharded optimizer
    fresh = Unsharded(name, cuda_device, world, mode, clip)
    for p, q in zip(fresh.params, sh.copies[0]):
        p.data.copy_(q.detach())
    fresh.opt.load_state_dict(full)
    # (b) the unsharded dictionary in fresh shards of another world, and (c) every rank's own shard dictionary in a fresh copy of it
    reshard, again = Sharded(name, cuda_device, 4, mode), Sharded(name, cuda_device, world, mode)
    for target in (reshard, again):
        for ps in target.copies:
            for p, q in zip(ps, ref.params):
                p.data.copy_(q.detach())
    for o in reshard.opts:
        o.load_state_dict(unsharded_dict)
    for o, d in zip(again.opts, shard_dicts):
        o.load_state_dict(d)
    ref.step(STEPS)
    fresh.step(STEPS)
    for target in (sh, reshard, again):
        target.step(STEPS, clip, expect=ref.params)
    for p, q in zip(fresh.params, ref.params):
        assert torch.equal(p.detach(), q.detach())
    want = ref.opt.state_dict()["state"]
    got = merge_shard_state_dicts([o.state_dict() for o in sh.opts])["state"]
    for other in (got, fresh.opt.state_dict()["state"], merge_shard_state_dicts([o.state_dict() for o in reshard.opts])["state"],
                  merge_shard_state_dicts([o.state_dict() for o in again.opts])["state"]):
        assert set(other) == set(want)
        for pid, st in want.items():
            for k, v in st.items():
                assert torch.equal(torch.as_tensor(v).cpu(), torch.as_tensor(other[pid][k]).cpu()), (pid, k)
            assert float(st["step"]) == STEPS + 1


def test_empty_shards_and_options(libprl, cuda_device):
    """A world larger than the slot count: the last ranks own nothing and still take part; master_weights=False with bf16
    parameters; a norm before the accumulators were reduced is refused."""
    from pipelinerl_amd.finetune.optim import FusedAdamW

    world = 4
    rng = np.random.default_rng(7)
    p0 = torch.from_numpy(rng.normal(0, 0.05, 17).astype(np.float32)).to(cuda_device, torch.bfloat16)
    g = torch.from_numpy(rng.normal(0, 1, 17).astype(np.float32)).to(cuda_device, torch.bfloat16)
    for master in (True, False):
        ref_p = torch.nn.Parameter(p0.clone())
        ref = FusedAdamW([ref_p], lr=1e-2, master_weights=master)
        copies = [torch.nn.Parameter(p0.clone()) for _ in range(world)]
        opts = [FusedAdamW([p], lr=1e-2, master_weights=master, shard=(r, world), grad_accum_dtype=torch.float32) for r, p in enumerate(copies)]
        assert [o.shard_len for o in opts] == [16] * world
        for _ in range(2):
            ref_p.grad = g.clone()
            ref.clip_and_step(1e6)
            for p, o in zip(copies, opts):
                p.grad = g.clone()
                o.accumulate_grads()
            with pytest.raises(RuntimeError, match="not reduced"):
                opts[0].local_grad_sumsq()
            total = sum(o.prepare_reduce() for o in opts)  # W equal terms, W a power of two: the average is the gradient itself
            for r, o in enumerate(opts):
                o.finish_reduce(total[r * 16:(r + 1) * 16])
            tot = sum(o.local_grad_sumsq().clone() for o in opts)
            for o in opts:
                o.norm_from_sumsq(tot, 1e6)
                o.step(clipped=True)
            gathered = torch.cat([o.pack_shard().clone() for o in opts])
            for o in opts:
                o.unpack_shards(gathered)
                o.zero_grad()
            assert _ulp_apart(opts[3]._record[0].cpu(), ref._record[0].cpu()) <= 1
            for p in copies:
                assert torch.equal(p.detach(), ref_p.detach())
        assert [len(o._table_params) for o in opts] == [1, 1, 0, 0] and not opts[2].state and not opts[3].state
        assert ("master" in opts[0].state[copies[0]]) == master and len(opts[0]._flat) == (3 if master else 2)
