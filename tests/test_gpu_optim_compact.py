"""The compact optimizer step (csrc/prl_optim_compact.hip: bf16 moments and / or bf16 parameters without a master copy, stored
with stochastic rounding) on the GPU: the kernel through the C ABI against the composition oracle of
tests/optim_compact_checks.py, the options of `FusedAdamW` / `FusedLion` (sharded = unsharded bit for bit, seeds, resuming, state
dictionaries across dtypes, state bytes), and the two unbiasedness experiments of tests/test_optim_compact_host.py on the device.

Acceptance against the oracle is per entry and per step, each step started from the device's own state so that one undecided
entry does not carry over: a bf16 store is DECIDED when no value within 4 fp32 ulp of the oracle's pre-rounding value rounds
differently - then it must be bit-equal - and must otherwise be one of the two neighbours; a value stored in fp32 must be within
those 4 ulp (the device's sqrt and divide may differ from the host's in the last ulps; the count that differs is printed).
Moments kept in fp32 also pass the per-entry bound of tests/optim_checks.py (fp64 witness, 4 x the fp32 CPU reference's error)."""

import copy

import numpy as np
import pytest
import torch

import optim_compact_checks as cc
from optim_checks import adamw_trajectory, check_entries, lion_trajectory, log_uniform_grads

pytestmark = pytest.mark.gpu

CHUNK = 16384
# edges of the group of 4, the lane group of 8, the chunk; then small parameters until the live segments need two launches (> 32)
SIZES = [1, 3, 4, 5, 7, 8, 9, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 12] + [2 + 3 * k for k in range(22)]
EMPTY, NOGRAD, VIEW = len(SIZES), len(SIZES) + 1, len(SIZES) + 2
NUMELS = SIZES + [0, 50, 1001]   # + one empty parameter, one without a gradient, one view offset by ONE element (scalar path)
PIECE = 9                        # this segment stands for the piece [16, 16 + n) of a larger parameter: elem_offset = 16
SLOT = 128                       # elements between two segments of a flat test buffer: 256-byte aligned for either dtype
SEED = 0xC0FFEE1234567
STEPS = 3
COEFS = [None, 0.37, None]       # the clip record: absent (coefficient 1) / < 1
TORCH_DT = {False: torch.float32, True: torch.bfloat16}


@pytest.fixture(scope="module")
def optmath(tmp_path_factory):
    return cc.build_optmath(tmp_path_factory.mktemp("compact_oracle"))


def _wd(i):
    return 0.01 if i % 2 == 0 else 0.0


def _offsets():
    offs, off = [], 0
    for i, n in enumerate(NUMELS):
        offs.append(off + (1 if i == VIEW else 0))
        off += -(-(n + 1) // SLOT) * SLOT
    return offs, off


def _flat(values, bf16, device, shifted):
    """One device buffer holding every segment's array (`values[i]`: fp32 numpy); `shifted`: the VIEW segment starts one element late."""
    offs, total = _offsets()
    host = np.zeros(total, np.float32)
    for i, v in enumerate(values):
        o = offs[i] - (0 if shifted or i != VIEW else 1)
        host[o:o + v.size] = v
    t = torch.from_numpy(host).to(device=device, dtype=TORCH_DT[bf16])
    return t, [offs[i] - (0 if shifted or i != VIEW else 1) for i in range(len(NUMELS))]


def _download(t):
    """fp32 values, or bf16 bit patterns as uint16."""
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def _edges():
    """First and last entry of every group of 4, lane group of 8, chunk and tensor (concatenated over the live segments)."""
    out = []
    for i, n in enumerate(NUMELS):
        if i in (EMPTY, NOGRAD):
            continue
        idx = np.arange(n)
        e = np.isin(idx % 8, (0, 3, 4, 7)) | (idx % CHUNK == 0) | (idx % CHUNK == CHUNK - 1)
        e[-1] = True
        out.append(e)
    return np.concatenate(out)


@pytest.mark.parametrize("state_bf16", [True, False], ids=["bf16state", "f32state"])
@pytest.mark.parametrize("grad_bf16", [True, False], ids=["bf16grad", "f32grad"])
@pytest.mark.parametrize("mode", ["f32", "master", "stochastic"])
@pytest.mark.parametrize("rule", ["adamw", "lion"])
def test_kernel_against_the_composition_oracle(libprl, cuda_device, optmath, rule, mode, grad_bf16, state_bf16):
    from pipelinerl_amd import _lib

    rng = np.random.default_rng(808)
    lr, betas = (1e-3, (0.9, 0.999)) if rule == "adamw" else (1e-4, (0.9, 0.99))
    param_bf16 = mode != "f32"

    def representable(a, bf16):
        return cc.widen(cc.rne(a)) if bf16 else a.astype(np.float32)

    p0 = [representable(rng.normal(0.0, 0.05, n), param_bf16) for n in NUMELS]
    m0 = [representable(rng.normal(0.0, 1e-3, n), state_bf16) for n in NUMELS]
    v0 = [representable(np.abs(rng.normal(0.0, 1e-3, n)) ** 2, state_bf16) for n in NUMELS]
    grads = [[representable(log_uniform_grads(rng, n, 1)[0], grad_bf16) for n in NUMELS] for _ in range(STEPS)]
    P, p_off = _flat(p0, param_bf16, cuda_device, shifted=True)
    M, s_off = _flat(m0, state_bf16, cuda_device, shifted=False)
    V, _ = _flat(v0, state_bf16, cuda_device, shifted=False)
    W, _ = _flat(p0, False, cuda_device, shifted=False)  # the master copies (mode "master")
    G = [_flat(g, grad_bf16, cuda_device, shifted=True)[0] for g in grads]
    assert (P.data_ptr() + p_off[VIEW] * P.element_size()) % 16 != 0 and (P.data_ptr() + p_off[0] * P.element_size()) % 16 == 0
    record = torch.zeros(2, dtype=torch.float32, device=cuda_device)
    live = [i for i in range(len(NUMELS)) if i not in (EMPTY, NOGRAD)]
    assert len(live) > 32 and len(NUMELS) >= 35, "the table takes two launches"
    edge = _edges()
    stream = _lib.current_stream_ptr(cuda_device)
    table = (_lib.PrlOptimCompactSegment * len(NUMELS))()
    frozen_before = [_download(t)[o[NOGRAD]:o[NOGRAD] + NUMELS[NOGRAD]].copy() for t, o in ((P, p_off), (M, s_off), (V, s_off))]
    for k in range(STEPS):
        step = k + 1
        before = {"param": _download(P), "exp_avg": _download(M), "exp_avg_sq": _download(V), "master": _download(W)}
        for i, n in enumerate(NUMELS):
            seg = table[i]
            seg.param, seg.numel, seg.param_dtype = P.data_ptr() + p_off[i] * P.element_size(), n, int(param_bf16)
            seg.grad = None if i == NOGRAD else G[k].data_ptr() + p_off[i] * G[k].element_size()
            seg.grad_dtype, seg.state_dtype = int(grad_bf16), int(state_bf16)
            seg.exp_avg = M.data_ptr() + s_off[i] * M.element_size()
            seg.exp_avg_sq = V.data_ptr() + s_off[i] * V.element_size() if rule == "adamw" else None
            seg.master = W.data_ptr() + s_off[i] * 4 if mode == "master" else None
            seg.param_rounding = _lib.PRL_ROUND_STOCHASTIC if mode == "stochastic" else _lib.PRL_ROUND_NEAREST
            seg.step, seg.lr, seg.weight_decay = step, lr, _wd(i)
            seg.elem_offset, seg.ordinal = (16 if i == PIECE else 0), i
        coef = COEFS[k]
        if coef is not None:
            record.copy_(torch.tensor([123.0, coef]))
        rec = record.data_ptr() if coef is not None else None
        if rule == "adamw":
            _lib.check(libprl.prl_optim_adamw_step_compact(table, len(NUMELS), betas[0], betas[1], 1e-8, SEED, rec, stream))
        else:
            _lib.check(libprl.prl_optim_lion_step_compact(table, len(NUMELS), betas[0], betas[1], SEED, rec, stream))
        torch.cuda.synchronize()
        after = {"param": _download(P), "exp_avg": _download(M), "exp_avg_sq": _download(V), "master": _download(W)}
        coef = 1.0 if coef is None else float(np.float32(coef))
        want, got = {}, {}
        moments = {key: ([], [], [], []) for key in ("exp_avg", "exp_avg_sq")}  # kernel, fp32 reference, fp64 witness, scale
        for i in live:
            n = NUMELS[i]
            cut = lambda name, off: before[name][off[i]:off[i] + n]  # noqa: E731
            oracle = cc.CompactOracle(optmath, rule, mode, state_bf16, cut("param", p_off), cut("exp_avg", s_off),
                                      cut("exp_avg_sq", s_off) if rule == "adamw" else None, cut("master", s_off) if mode == "master" else None,
                                      lr=lr, wd=_wd(i), betas=betas, seed=SEED, ordinal=i, elem_offset=16 if i == PIECE else 0)
            w_in = oracle.master.copy() if mode == "master" else oracle._f32(oracle.p)
            m_in, v_in = oracle._f32(oracle.m), (oracle._f32(oracle.v) if rule == "adamw" else None)
            for name, st in oracle.step(grads[k][i], coef, step).items():
                want.setdefault(name, []).append(st)
                off = p_off if name == "param" else s_off
                got.setdefault(name, []).append(after[name][off[i]:off[i] + n])
            if not state_bf16:  # the parent's per-entry bound on the fp32 moments, one step from the device's own state
                if rule == "adamw":
                    ref, _ = adamw_trajectory(w_in, [grads[k][i]], [coef], lr, _wd(i), betas=betas, dtype=torch.float32, m0=m_in, v0=v_in, step0=k)
                    wit, scales = adamw_trajectory(w_in, [grads[k][i]], [coef], lr, _wd(i), betas=betas, dtype=torch.float64, m0=m_in, v0=v_in, step0=k)
                    for q, key in ((1, "exp_avg"), (2, "exp_avg_sq")):
                        for lst, val in zip(moments[key], (got[key][-1], ref[0][q], wit[0][q], scales[0][q])):
                            lst.append(val)
                else:
                    ref, _ = lion_trajectory(w_in, m_in, [grads[k][i]], [coef], lr, _wd(i), betas=betas, dtype=np.float32)
                    wit, scales = lion_trajectory(w_in, m_in, [grads[k][i]], [coef], lr, _wd(i), betas=betas, dtype=np.float64)
                    for lst, val in zip(moments["exp_avg"], (got["exp_avg"][-1], ref[0][1], wit[0][1], scales[0][1])):
                        lst.append(val)
        tag = f"{rule} {mode} grad {'bf16' if grad_bf16 else 'f32'} state {'bf16' if state_bf16 else 'f32'} step {step}"
        assert set(want) == {"param", "exp_avg"} | ({"exp_avg_sq"} if rule == "adamw" else set()) | ({"master"} if mode == "master" else set())
        for name, parts in want.items():
            addend = None if parts[0].addend is None else np.concatenate([s.addend for s in parts])
            whole = cc.Stored(np.concatenate([s.pre for s in parts]), addend, np.concatenate([s.out for s in parts]))
            cc.check_store(f"{tag} {name}", np.concatenate(got[name]), whole, edge=edge)
        for key, (K, R, Wt, S) in moments.items():
            if K:
                r = check_entries(f"{tag} {key} (fp32 state)", np.concatenate(K), np.concatenate(R), np.concatenate(Wt), np.concatenate(S))
                check_entries(f"{tag} {key} (fp32 state, group / chunk / tensor edges)", np.concatenate(K)[edge], np.concatenate(R)[edge],
                              np.concatenate(Wt)[edge], np.concatenate(S)[edge], r_ref=r)
        # nothing outside the segments moved: the padding between them, the element in front of the shifted view, the arrays a mode does not own
        for name, off in (("param", p_off), ("exp_avg", s_off), ("exp_avg_sq", s_off), ("master", s_off)):
            mask = np.ones(before[name].size, dtype=bool)
            owned = name in want
            for i in live:
                if owned:
                    mask[off[i]:off[i] + NUMELS[i]] = False
            assert np.array_equal(before[name][mask], after[name][mask]), f"{tag}: {name} was written outside its segments"
    for (t, o), was in zip(((P, p_off), (M, s_off), (V, s_off)), frozen_before):
        assert np.array_equal(_download(t)[o[NOGRAD]:o[NOGRAD] + NUMELS[NOGRAD]], was), "no gradient: parameter and state untouched"


# ---- through FusedAdamW / FusedLion -------------------------------------------------------------------------------------
P_NUMELS = [5, CHUNK, CHUNK + 1, 2 * CHUNK + 12, 0, 7, 1, 15, 16, 17, 33, 64]
P_BF16 = {0, 1, 2, 3, 6, 8, 10}
CONFIGS = {  # constructor options
    "compact": dict(state_dtype=torch.bfloat16, param_rounding="stochastic", master_weights=False),
    "bf16state+master": dict(state_dtype=torch.bfloat16, master_weights=True),
    "f32state+sr": dict(param_rounding="stochastic", master_weights=False),
}
MAX_WORLD = 3


def _cls(rule):
    from pipelinerl_amd.finetune import optim

    return {"adamw": optim.FusedAdamW, "lion": optim.FusedLion}[rule]


def _lr(rule):
    return {"adamw": 1e-3, "lion": 1e-4}[rule]


def _pdtype(i):
    return torch.bfloat16 if i in P_BF16 else torch.float32


_DATA = {}


def _data():
    """(p0[i], grads[step][rank][i]) as fp32 numpy holding values the parameter's dtype represents; computed once."""
    if not _DATA:
        rng = np.random.default_rng(9090)
        cut = lambda a, i: torch.from_numpy(a.astype(np.float32)).to(_pdtype(i)).float().numpy()  # noqa: E731
        _DATA["p0"] = [cut(rng.normal(0.0, 0.05, n), i) for i, n in enumerate(P_NUMELS)]
        _DATA["grads"] = [[[cut(log_uniform_grads(rng, n, 1)[0], i) for i, n in enumerate(P_NUMELS)] for _ in range(MAX_WORLD)] for _ in range(STEPS + 1)]
    return _DATA["p0"], _DATA["grads"]


def _params(device):
    return [torch.nn.Parameter(torch.from_numpy(a).to(device=device, dtype=_pdtype(i))) for i, a in enumerate(_data()[0])]


def _groups(params):
    return [{"params": params[0::2], "weight_decay": 0.01}, {"params": params[1::2], "weight_decay": 0.0}]


def _grad(step, rank, i, device):
    return torch.from_numpy(_data()[1][step][rank][i]).to(device=device, dtype=_pdtype(i))


def _bits(t):
    if t.numel() == 0:
        return torch.empty(0, dtype=torch.uint8, device=t.device)
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


class Run:
    """One unsharded optimizer with fp32 accumulation: two micro-batches (the draws of ranks 0 and 1) are folded, then clip_and_step."""

    def __init__(self, rule, device, **kw):
        self.params = _params(device)
        self.opt = _cls(rule)(_groups(self.params), lr=_lr(rule), grad_accum_dtype=torch.float32, **kw)
        self.device = device

    def step(self, s, max_norm=0.05):
        for micro in range(2):
            for i, p in enumerate(self.params):
                p.grad = _grad(s, micro, i, self.device)
            self.opt.accumulate_grads()
        norm = self.opt.clip_and_step(max_norm)
        self.opt.zero_grad()
        return norm


def _assert_same(a: Run, b: Run, what):
    for i, (p, q) in enumerate(zip(a.params, b.params)):
        assert torch.equal(_bits(p), _bits(q)), f"{what}: parameter {i}"
        sa, sb = a.opt.state[p], b.opt.state[q]
        assert set(sa) == set(sb)
        for k in sa:
            assert sa[k].dtype == sb[k].dtype and torch.equal(_bits(sa[k].to(p.device)), _bits(sb[k].to(p.device))), f"{what}: {k} of parameter {i}"


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("rule", ["adamw", "lion"])
def test_seeds_resume_and_state_dtypes(libprl, cuda_device, rule, config):
    kw = CONFIGS[config]
    a, b, c = Run(rule, cuda_device, seed=11, **kw), Run(rule, cuda_device, seed=11, **kw), Run(rule, cuda_device, seed=12, **kw)
    for s in range(2):
        assert float(a.step(s)) > 0.05, "the clip is engaged"
        b.step(s)
        c.step(s)
    saved = copy.deepcopy(a.opt.state_dict())
    assert all(g["seed"] == 11 for g in saved["param_groups"])
    resumed = Run(rule, cuda_device, seed=999, **kw)  # the saved seed replaces this one
    for p, q in zip(resumed.params, a.params):
        p.data.copy_(q.detach())
    resumed.opt.load_state_dict(saved)
    for r in (a, b, c, resumed):
        r.step(2)
    _assert_same(a, b, "two runs with one seed")
    _assert_same(a, resumed, "resumed after step 2 from state_dict()")
    differs = [i for i, (p, q) in enumerate(zip(a.params, c.params))
               if not torch.equal(_bits(p), _bits(q)) or not torch.equal(_bits(a.opt.state[p]["exp_avg"]), _bits(c.opt.state[q]["exp_avg"]))]
    assert set(differs) >= {i for i in P_BF16 if P_NUMELS[i] >= CHUNK}, "another seed rounds differently (parameter or exp_avg of every large bf16 parameter)"
    # dtypes and bytes of the state
    sdt = kw.get("state_dtype", torch.float32)
    keys = a.opt._state_keys
    for i, p in enumerate(a.params):
        st = a.opt.state[p]
        assert float(st["step"]) == 3 and all(st[k].dtype == sdt and st[k].shape == p.shape for k in keys)
        assert ("master" in st) == (kw["master_weights"] and i in P_BF16) and ("master" not in st or st["master"].dtype == torch.float32)
        if i in P_BF16 and "master" in st:
            assert torch.equal(_bits(p), _bits(st["master"].to(torch.bfloat16))), "with a master copy the parameter stays its nearest image"
        per_element = sum(st[k].element_size() for k in st if k != "step")
        want = len(keys) * (2 if sdt == torch.bfloat16 else 4) + (4 if "master" in st else 0)
        assert per_element == want
        if config == "compact" and i in P_BF16:
            assert per_element == (4 if rule == "adamw" else 2), "AdamW: 4 bytes of state per bf16 element, Lion: 2"
    slots = sum(-(-n // 16) * 16 for n in P_NUMELS)
    flat_bytes = sum(f.numel() * f.element_size() for f in a.opt._flat)
    master_slots = sum(-(-n // 16) * 16 for i, n in enumerate(P_NUMELS) if i in P_BF16) if kw["master_weights"] else 0
    assert flat_bytes == slots * len(keys) * (2 if sdt == torch.bfloat16 else 4) + master_slots * 4
    sd = a.opt.state_dict()
    assert all(sd["state"][pid][k].dtype == sdt for pid in sd["state"] for k in keys), "state_dict() holds the moments in state_dtype"
    # a dictionary of the other state dtype loads: bf16 -> fp32 exactly, fp32 -> bf16 to nearest even
    other_dt = torch.float32 if sdt == torch.bfloat16 else torch.bfloat16
    other = Run(rule, cuda_device, **{**kw, "state_dtype": other_dt})
    for p, q in zip(other.params, a.params):
        p.data.copy_(q.detach())
    other.opt.load_state_dict(copy.deepcopy(sd))
    order = list(range(0, len(P_NUMELS), 2)) + list(range(1, len(P_NUMELS), 2))  # state_dict() numbers the parameters in param_groups order
    for pid, i in enumerate(order):
        p = other.params[i]
        for k in keys:
            got = other.opt.state[p][k]
            assert got.dtype == other_dt and torch.equal(_bits(got), _bits(sd["state"][pid][k].to(device=p.device, dtype=other_dt))), (pid, k)
    other.step(3)
    assert all(other.opt.state[p][k].dtype == other_dt and float(other.opt.state[p]["step"]) == 4 for p in other.params for k in keys)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("rule", ["adamw", "lion"])
def test_sharded_stand_ins_are_bit_equal_to_the_unsharded_run(libprl, cuda_device, rule, config, world):
    """`shard=(r, w)` stand-ins with fp32 accumulation, the collectives by hand as in tests/test_gpu_optim_sharded.py; the clip is not
    engaged (the norm of shard sums may differ from the unsharded one in the last ulp, the coefficient 1 cannot)."""
    from pipelinerl_amd.finetune.optim import merge_shard_state_dicts

    kw = dict(CONFIGS[config], seed=21)
    ref_params = _params(cuda_device)
    ref = _cls(rule)(_groups(ref_params), lr=_lr(rule), grad_accum_dtype=torch.float32, **kw)
    copies = [_params(cuda_device) for _ in range(world)]
    opts = [_cls(rule)(_groups(ps), lr=_lr(rule), grad_accum_dtype=torch.float32, shard=(r, world), **kw) for r, ps in enumerate(copies)]
    for s in range(STEPS):
        # unsharded: the average the ranks' accumulators reduce to (their sum in rank order over the world size), as an fp32 gradient
        for i, p in enumerate(ref_params):
            total = _grad(s, 0, i, cuda_device).float()
            for r in range(1, world):
                total = total + _grad(s, r, i, cuda_device).float()
            if p.dtype != torch.float32:
                p.grad_dtype = torch.float32
            p.grad = total / world
        ref.accumulate_grads()
        ref.clip_and_step(1e6)
        assert float(ref._record[1]) == 1.0
        ref.zero_grad()
        for r, (ps, o) in enumerate(zip(copies, opts)):
            for i, p in enumerate(ps):
                p.grad = _grad(s, r, i, cuda_device)
            o.accumulate_grads()
        flats = [o.prepare_reduce() for o in opts]
        total = flats[0].clone()
        for f in flats[1:]:
            total += f
        for r, o in enumerate(opts):
            o.finish_reduce(total[r * o.shard_len:(r + 1) * o.shard_len])
        parts = [o.local_grad_sumsq().clone() for o in opts]
        tot = parts[0].clone()
        for x in parts[1:]:
            tot += x
        for o in opts:
            o.norm_from_sumsq(tot, 1e6)
            assert float(o._record[1]) == 1.0
            o.step(clipped=True)
        gathered = torch.cat([o.pack_shard().clone() for o in opts])
        for o in opts:
            o.unpack_shards(gathered)
            o.zero_grad()
        for r, ps in enumerate(copies):
            for i, (p, q) in enumerate(zip(ps, ref_params)):
                assert torch.equal(_bits(p), _bits(q)), f"step {s}: parameter {i} on rank {r} of {world}"
    merged = merge_shard_state_dicts([o.state_dict() for o in opts])["state"]
    want = ref.state_dict()["state"]
    assert set(merged) == set(want)
    sdt = kw.get("state_dtype", torch.float32)
    for pid, st in want.items():
        assert set(st) == set(merged[pid])
        for k, v in st.items():
            a, b = torch.as_tensor(v), torch.as_tensor(merged[pid][k])
            assert a.dtype == b.dtype and torch.equal(_bits(a.cpu()), _bits(b.cpu())), (pid, k)
            if k in ref._state_keys:
                assert a.dtype == sdt
    for o in opts:  # allocation: the own range only, in the state dtype
        n_master = 1 if kw["master_weights"] else 0
        assert sum(f.numel() * f.element_size() for f in o._flat) == o.shard_len * (len(o._state_keys) * (2 if sdt == torch.bfloat16 else 4) + 4 * n_master)


# ---- unbiasedness on the device -------------------------------------------------------------------------------------------
def test_parameter_drift_is_unbiased_on_the_device(libprl, cuda_device):
    from pipelinerl_amd.finetune.optim import FusedAdamW

    e = cc.DRIFT
    ones = torch.ones(e["n"], dtype=torch.bfloat16, device=cuda_device)
    g = torch.full((e["n"],), e["g"], dtype=torch.bfloat16, device=cuda_device)
    p, q = torch.nn.Parameter(ones.clone()), torch.nn.Parameter(ones.clone())
    compact = FusedAdamW([p], lr=e["lr"], weight_decay=0.0, master_weights=False, state_dtype=torch.bfloat16, param_rounding="stochastic", seed=0)
    nearest = FusedAdamW([q], lr=e["lr"], weight_decay=0.0, master_weights=False)
    p.grad, q.grad = g, g.clone()
    for _ in range(e["steps"]):
        compact.step()
        nearest.step()
    assert torch.equal(q.detach(), ones), "master_weights=False with round-to-nearest: every update is rounded away"
    assert compact.state[p]["exp_avg"].dtype == torch.bfloat16 and compact.state[p]["exp_avg_sq"].dtype == torch.bfloat16
    cc.assert_within_standard_errors("device parameter drift", p.detach().float().cpu().numpy(), cc.adamw_witness_fp64(e["p0"], e["g"], e["lr"], e["steps"]))


def test_second_moment_decay_is_unbiased_on_the_device(libprl, cuda_device):
    from pipelinerl_amd.finetune.optim import FusedAdamW

    e = cc.DECAY
    n = e["n"]
    p = torch.nn.Parameter(torch.ones(n, dtype=torch.bfloat16, device=cuda_device))
    opt = FusedAdamW([p], lr=1e-5, betas=(0.9, e["beta2"]), weight_decay=0.0, master_weights=False, state_dtype=torch.bfloat16, param_rounding="stochastic", seed=0)
    sd = opt.state_dict()
    sd["state"] = {0: {"step": torch.tensor(0.0), "exp_avg": torch.zeros(n), "exp_avg_sq": torch.full((n,), e["v0"])}}  # fp32 1.0 -> bf16 1.0, exactly
    opt.load_state_dict(sd)
    p.grad = torch.zeros(n, dtype=torch.bfloat16, device=cuda_device)
    for _ in range(e["steps"]):
        opt.step()
    st = opt.state[p]
    assert st["exp_avg_sq"].dtype == torch.bfloat16 and float(st["step"]) == e["steps"]
    assert torch.equal(p.detach(), torch.ones_like(p)) and not st["exp_avg"].any(), "zero gradient: nothing else moves"
    # (round-to-nearest leaves 1.0, asserted on the host in tests/test_optim_compact_host.py: the product has no nearest bf16 state to run here)
    cc.assert_within_standard_errors("device second-moment decay", st["exp_avg_sq"].float().cpu().numpy(), e["beta2"] ** e["steps"])
