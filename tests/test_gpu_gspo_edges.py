"""The sequence-level (GSPO) path at the edges of its own kernels: `gspo_segment_sums_kernel` / `gspo_order_check_kernel` /
`gspo_segment_terms_kernel` / `gspo_expand_kernel` through the C ABI (so that `sums`, `coef` and `indicator` are visible), the
wrapper `gspo_segment_terms`, the GSPO instantiations of `grpo_loss_partial_kernel`, and `rl_step` / `rl_step_fused_head` on top.

Every per-segment number is compared with the fp64 witness of tests/seq_term_checks.py: the sums under the derived fp64 bound,
`coef` per segment and the loss under COEF_BOUND / LOSS_BOUND (4 x the oracle's own fp32 error, measured on the CPU by
tests/test_seq_term_checks_host.py on the cases built HERE), `indicator` and the per-token columns bit for bit.

Paths no other test reaches, and the case that reaches each:
  * a run longer than one trip of the 256-thread strided loop (257 .. 8192 tokens), a run that is empty because the segment
    owns column 0 only, `n_segments` above the largest id present                                  (test_run_geometry)
  * more than 256 segments in the one-workgroup terms kernel; more than 4096 x 256 columns in the expand kernel's capped grid
                                                                                                    (test_many_segments)
  * a ratio exactly on both clip bounds (tie rule, inclusive inside rule), every side of the clip x sign of the advantage
                                                                                                    (test_clip_edges)
  * a slice that starts at segment 3 with pre-reduced sums and grad_scale 2; zero_out             (test_slice_form)
  * the GSPO order check: unsorted ids, an id outside [0, n_segments) on a labelled / unlabelled token (test_order_check)
  * `grpo_loss_partial_kernel<1, false, true>` (misaligned views) and the T % 4 tails under GSPO   (test_k2_under_gspo)
"""

import ctypes
import dataclasses
import functools
import types

import numpy as np
import pytest
import torch

from oracle import rl_loss as orl

import grad_checks as gc
import seq_term_checks as sc

pytestmark = pytest.mark.gpu

FP_TOL = 1e-4  # the suite's tolerance for statistics
F32 = np.float32
RATIOS = (0.90, 0.97, 1.0, 1.03, 1.10)  # every one at least 2 % from the clip bounds 0.95 / 1.05
EXPAND_GRID_COLUMNS = 4096 * 256        # gspo_expand_kernel: at most 4096 workgroups of 256 threads, then it strides


def loss_cfg(group_normalization=False, overlong_filtering=False, eps=0.05, **kw):
    return dict(policy_loss="gspo", epsilon_low=eps, epsilon_high=eps, kl_coef=0.05, final_kl_coef=0.05, batch_size=16,
                group_normalization=group_normalization, overlong_filtering=overlong_filtering, divide_advantage_by_std=False, **kw)


ALL_CFGS = [loss_cfg(g, o) for g in (False, True) for o in (False, True)]


# ---- inputs (pure host code; tests/test_seq_term_checks_host.py measures the oracle on the same arrays) --------------------
def seg(n, lab="all", ratio=1.0, adv=1.0, ovf=0):
    """One segment: length, labelled pattern (all / none / first / last / random), target exp(mean log-ratio), mean advantage,
    overflow flag."""
    return dict(n=int(n), lab=lab, ratio=float(ratio), adv=float(adv), ovf=int(ovf))


def build(segs, seed, vocab=1031, new=None, exact=False, first_id=0):
    """Lay the columns of one packed row out ([1, T] numpy, the fields of PipelineBatchEncoding + `new_logprobs`).  Within a
    segment new - old is noise (sigma 0.05) around the target, shifted until the fp64 mean of the fp32 differences over the
    labelled tokens hits the target to ~1e-9.  `new` [T]: log-probs given from outside (a model's), then `old` is solved for.
    `exact`: new == old on every token (ratio exactly 1)."""
    rng = np.random.default_rng(seed)
    T = sum(s["n"] for s in segs)
    cols = {k: np.zeros(T, dtype=F32) for k in ("new_logprobs", "old_logprobs", "ref_logprobs", "advantages", "rewards", "group_tokens",
                                                "num_labels", "overflow")}
    ids = rng.integers(0, vocab, size=T).astype(np.int64)
    labels = ids.copy()
    seg_ids, pos = np.zeros(T, dtype=np.int64), np.zeros(T, dtype=np.int64)
    a = 0
    for i, s in enumerate(segs):
        n = s["n"]
        sl = slice(a, a + n)
        lab = np.zeros(n, dtype=bool)
        if s["lab"] == "all":
            lab[:] = True
        elif s["lab"] == "first":
            lab[0] = True
        elif s["lab"] == "last":
            lab[-1] = True
        elif s["lab"] == "random":
            lab = rng.random(n) < 0.8
            lab[rng.integers(0, n)] = True
        labels[sl][~lab] = -100
        counted = lab & (np.arange(a, a + n) > 0)  # column 0 predicts nothing
        d = rng.normal(0.0, 0.05, n)
        if new is None:
            fixed = rng.uniform(-3.0, -0.05, n).astype(F32)  # old
        else:
            fixed = np.asarray(new[sl], dtype=F32)
        if exact:
            other = fixed.copy()
        else:
            for _ in range(6):
                other = (fixed.astype(np.float64) + d).astype(F32) if new is None else (fixed.astype(np.float64) - d).astype(F32)
                actual = ((other - fixed) if new is None else (fixed - other)).astype(F32).astype(np.float64)
                if counted.any():
                    d = d + (np.log(s["ratio"]) - actual[counted].mean())
        cols["new_logprobs"][sl], cols["old_logprobs"][sl] = (other, fixed) if new is None else (fixed, other)
        adv = rng.normal(0.0, 1.0, n)  # unlabelled tokens carry values too: a mask that fails shows
        if s["adv"] == 0.0:
            adv[lab] = 0.0
        else:
            adv[lab] = s["adv"] * (1.0 + 0.1 * rng.normal(0.0, 1.0, int(lab.sum())))
        cols["advantages"][sl] = adv
        cols["ref_logprobs"][sl] = cols["old_logprobs"][sl] + rng.normal(0.0, 0.05, n)
        cols["rewards"][sl] = float(rng.integers(0, 2))
        cols["group_tokens"][sl] = float(rng.integers(20, 5000))
        cols["num_labels"][sl] = float(max(int(lab.sum()), 1))
        cols["overflow"][sl] = float(s["ovf"])
        seg_ids[sl], pos[sl] = first_id + i, np.arange(n)
        a += n
    batch = {k: v[None] for k, v in cols.items()}
    batch.update(input_ids=ids[None], labels=labels[None], attention_mask=np.ones((1, T), dtype=np.int64), position_ids=pos[None],
                 segment_ids=seg_ids[None], model_version=0, is_packed=True)
    batch["entropy"] = rng.uniform(0.5, 3.0, (1, T)).astype(F32)  # token-aligned stand-in for the statistics of K2
    return batch


def _fill(rng, count, lo=1, hi=70):
    """`count` ordinary segments of lo .. hi tokens: random labels, ratios from RATIOS, advantages of either sign."""
    return [seg(rng.integers(lo, hi + 1), rng.choice(["all", "random"]), rng.choice(RATIOS), rng.choice([-1.0, 1.0]) * rng.uniform(0.2, 2.0))
            for _ in range(count)]


def geometry_segments():
    rng = np.random.default_rng(11)
    f = _fill(rng, 36)
    f[3], f[7], f[15], f[20] = seg(23, "none", 1.10, 1.0), seg(31, "first", 0.97, -1.0), seg(29, "last", 1.03, 1.0), seg(40, "all", 0.97, 1.0, ovf=1)
    # segment 0 owns column 0 only: its run in [1, cols) is empty.  Lengths around the 256-thread trip of the sums kernel;
    # the 8192-token run sits between neighbours on the other sides of the clip range
    return ([seg(1, "all", 1.0, 1.0), seg(2, "all", 0.97, 1.0), seg(3, "all", 1.03, -1.0)] + f[:12]
            + [seg(255, "all", 0.97, 1.0), seg(256, "random", 1.10, -1.0), seg(257, "all", 1.03, 1.0)] + f[12:24]
            + [seg(511, "random", 0.90, 1.0), seg(8192, "all", 1.03, 1.0), seg(512, "all", 1.10, 1.0)] + f[24:]
            + [seg(513, "random", 1.0, -1.0)])


def e2e_segments(total=2048):
    """The head of the run-geometry case, cut to `total` tokens (the last segment shortened to fit)."""
    out, n = [], 0
    for s in geometry_segments():
        if n + s["n"] >= total:
            out.append(dict(s, n=total - n))
            break
        out.append(s)
        n += s["n"]
    return out


def many_segments():
    rng = np.random.default_rng(12)
    out = _fill(rng, 700, 1, 5)
    for i in range(5, 700, 37):
        out[i] = seg(out[i]["n"], "none", 1.0, 1.0)
    return out


def wide_segments():
    rng = np.random.default_rng(13)
    out = [seg(n, "random", rng.choice(RATIOS), rng.choice([-1.0, 1.0]) * rng.uniform(0.2, 2.0)) for n in rng.integers(4000, 4400, 300)]
    assert sum(s["n"] for s in out) >= 1_200_000 > EXPAND_GRID_COLUMNS
    return out


def clip_segments():
    rng = np.random.default_rng(14)
    return [seg(1, "all", 1.0, 1.0)] + [seg(rng.integers(5, 40), "all", r, a) for r in RATIOS for a in (0.8, -0.8, 0.0)]


def tie_segments():
    return [seg(1, "all"), seg(17, "all", adv=0.7), seg(9, "random", adv=-0.7), seg(30, "all", adv=0.0), seg(300, "all", adv=1.3), seg(5, "none")]


SLICE_FIRST, SLICE_SEGMENTS = 3, 9


def slice_segments():
    # the clip indicator alternates 1, 0, 1, ...: indexing it by seg instead of seg - seg[0] gives the wrong one on every token
    r = (1.10, 1.0, 0.90, 1.0, 1.10, 1.03, 0.90, 0.97, 1.10)
    return [seg(20 + 9 * i, "random", r[i], (-1.0) ** i * 0.9) for i in range(SLICE_SEGMENTS)]


def nan_segments():
    return [seg(1, "all")] + [seg(12 + i, "all", RATIOS[i], 1.0 - 0.5 * i) for i in range(5)]


@functools.lru_cache(maxsize=None)
def case(name: str):
    """name -> (batch, loss configs, extras).  Every case has its own seed."""
    if name == "geometry":
        return build(geometry_segments(), 101), ALL_CFGS, {}
    if name == "many":
        return build(many_segments(), 102), [loss_cfg(True, False)], {}
    if name == "wide":
        return build(wide_segments(), 103), [loss_cfg(False, False)], {}
    if name == "clip":
        return build(clip_segments(), 104), [loss_cfg(), loss_cfg(True, True)], {}
    if name == "tie":
        return build(tie_segments(), 105, exact=True), [loss_cfg(eps=0.0), loss_cfg(True, False, eps=0.0)], {}
    if name == "slice":
        whole = build(slice_segments(), 106)
        start = int(np.flatnonzero(whole["segment_ids"][0] == SLICE_FIRST)[0]) + 7  # inside segment 3
        part = {k: (v[:, start:] if isinstance(v, np.ndarray) else v) for k, v in whole.items()}
        assert part["segment_ids"][0, 0] == SLICE_FIRST
        return part, [loss_cfg(), loss_cfg(True, False)], {"whole": whole, "grad_scale": 2.0}
    if name == "nan":
        b = build(nan_segments(), 107)
        u = int(np.flatnonzero(b["segment_ids"][0] == 2)[3])
        assert b["labels"][0, u] != -100
        b["new_logprobs"][0, u] = np.nan
        return b, [loss_cfg()], {"nan_segment": 2}
    if name == "e2e":
        logits, new = e2e_logits()
        return build(e2e_segments(), 108, new=new), [loss_cfg()], {"logits": logits}
    raise KeyError(name)


CASE_NAMES = ("geometry", "many", "wide", "clip", "tie", "slice", "nan", "e2e")
E2E_T, E2E_V = 2048, 1031


@functools.lru_cache(maxsize=1)
def e2e_logits():
    """(logits [1, T, V] = 2 * randn, the fp32 log-probs of the tokens the e2e case is built with, token-aligned [T])."""
    g = torch.Generator().manual_seed(108)
    logits = (torch.randn(1, E2E_T, E2E_V, generator=g) * 2).numpy()
    ids = build(e2e_segments(), 108)["input_ids"]  # the ids depend on the seed only
    nlp64, _, _ = gc.forward_witness(logits[0, :-1], ids[0, 1:], 1.0)
    return logits, np.concatenate([[0.0], nlp64]).astype(F32)


def columns(batch):
    """The witness's positional arguments."""
    return tuple(batch[k] for k in ("segment_ids", "labels", "new_logprobs", "old_logprobs", "advantages", "group_tokens", "overflow"))


def oracle_terms(batch, cfg, grad_scale=1.0):
    """The oracle's fp32 GSPO branch on a whole packed row -> (coef [S] x grad_scale, loss, its clip statistic): `coef` is
    read off `g_nlp` at a labelled token of each segment (a segment without one has no observable coefficient: 0)."""
    res = orl.token_loss(batch, batch["new_logprobs"][:, 1:], batch["entropy"][:, 1:], cfg, 0, 10, True)
    sid, lab = batch["segment_ids"][0, 1:], batch["labels"][0, 1:] != -100
    coef = np.zeros(int(batch["segment_ids"].max()) + 1)
    u = np.flatnonzero(lab)
    coef[sid[u]] = res["g_nlp"][0, u].astype(np.float64) * grad_scale  # every labelled token of a segment holds the same value
    return coef, float(res["loss"]), res


# ---- device side -------------------------------------------------------------------------------------------------------------
SENTINEL = -7.0  # what the output buffers hold before a launch: an entry nobody wrote cannot pass for a result


def _c_cfg(cfg):
    from pipelinerl_amd.finetune.rl import RLConfig, make_loss_config

    return make_loss_config(RLConfig(**cfg), 0, 10)[0]


def _dev(batch, dev, keys=("segment_ids", "labels", "new_logprobs", "old_logprobs", "advantages", "group_tokens", "overflow")):
    return {k: torch.from_numpy(np.ascontiguousarray(batch[k])).to(dev) for k in keys}


def run_sums(lib, c_cfg, d, n_seg):
    from pipelinerl_amd import _lib

    dev = d["labels"].device
    cols = d["labels"].shape[-1]
    assert all(t.is_contiguous() and t.shape[-1] == cols for t in d.values())
    sums = torch.full((4, n_seg), SENTINEL, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.prl_gspo_segment_sums(ctypes.byref(c_cfg), cols, n_seg, _lib.ptr(d["segment_ids"]), _lib.ptr(d["labels"]),
                                             _lib.ptr(d["new_logprobs"]), _lib.ptr(d["old_logprobs"]), _lib.ptr(d["advantages"]),
                                             _lib.ptr(d["group_tokens"]), _lib.ptr(d["overflow"]), _lib.ptr(sums), _lib.current_stream_ptr(dev)))
    return sums


def run_terms(lib, c_cfg, sums, grad_scale=1.0, zero_out=0):
    from pipelinerl_amd import _lib

    dev, n_seg = sums.device, sums.shape[1]
    assert sums.is_contiguous() and sums.dtype == torch.float64 and sums.shape[0] == 4
    coef = torch.full((n_seg,), SENTINEL, dtype=torch.float32, device=dev)
    ind = torch.full_like(coef, SENTINEL)
    loss = torch.full((), SENTINEL, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.prl_gspo_segment_terms(ctypes.byref(c_cfg), n_seg, _lib.ptr(sums), float(grad_scale), int(zero_out), _lib.ptr(coef),
                                              _lib.ptr(ind), _lib.ptr(loss), _lib.current_stream_ptr(dev)))
    return coef, ind, loss


def run_expand(lib, seg_ids, coef, ind):
    from pipelinerl_amd import _lib

    dev, cols = seg_ids.device, seg_ids.shape[-1]
    assert seg_ids.is_contiguous() and coef.shape == ind.shape and coef.numel() >= 1
    ext_g = torch.full((1, cols), SENTINEL, dtype=torch.float32, device=dev)
    ext_c = torch.full_like(ext_g, SENTINEL)
    with torch.cuda.device(dev):
        _lib.check(lib.prl_gspo_expand(cols, coef.numel(), _lib.ptr(seg_ids), _lib.ptr(coef), _lib.ptr(ind), _lib.ptr(ext_g), _lib.ptr(ext_c),
                                       _lib.current_stream_ptr(dev)))
    return ext_g, ext_c


def _np(t):
    return t.detach().cpu().numpy()


def run_all(lib, dev, batch, cfg, n_seg=None, sums=None, grad_scale=1.0, zero_out=0):
    """The three entry points in the wrapper's order -> numpy (sums, coef, indicator, loss, ext_g, ext_c)."""
    c_cfg = _c_cfg(cfg)
    d = _dev(batch, dev)
    n_seg = int(batch["segment_ids"].max()) + 1 if n_seg is None else n_seg
    own = run_sums(lib, c_cfg, d, n_seg)
    used = own if sums is None else torch.from_numpy(np.ascontiguousarray(sums, dtype=np.float64)).to(dev)
    coef, ind, loss = run_terms(lib, c_cfg, used, grad_scale, zero_out)
    ext_g, ext_c = run_expand(lib, d["segment_ids"], coef, ind)
    torch.cuda.synchronize()
    return tuple(_np(t) for t in (own, coef, ind, loss, ext_g, ext_c))


def assert_checks(label, batch, cfg, got, w, sums_witness=None):
    """Sums under the derived bound, coef / indicator / loss under the table's bounds, every token bit for bit."""
    sums, coef, ind, loss, ext_g, ext_c = got
    rs = sc.check_sums(sums, sums_witness or w)
    rt = sc.check_terms(coef, ind, loss, w)
    bad, at = sc.check_tokens(ext_g, ext_c, batch["segment_ids"], coef, ind)
    print(f"{label}: sums {rs.worst:.3f} x derived bound; coef {rt.coef_err:.3e} (bound {sc.COEF_BOUND:.1e}); "
          f"loss {rt.loss_err:.3e} (bound {sc.LOSS_BOUND:.1e}); {bad} of {ext_g.size} tokens differ")
    assert rs.ok(), f"{label}: {rs}"
    assert rt.ok(), f"{label}: {rt}"
    assert bad == 0, f"{label}: {bad} tokens of ext_g / ext_c differ from the per-token rule, first at column {at}"
    return rs, rt


def _cfg_id(cfg):
    return f"gn{int(cfg['group_normalization'])}_of{int(cfg['overlong_filtering'])}_eps{cfg['epsilon_low']}"


def _pb(batch, dev):
    from pipelinerl_amd.finetune.types import PipelineBatchEncoding

    fields = {k: (torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v) for k, v in batch.items()
              if k not in ("new_logprobs", "entropy")}
    return PipelineBatchEncoding(**fields).to_device(dev)


@pytest.mark.parametrize("cfg", ALL_CFGS, ids=_cfg_id)
def test_run_geometry(libprl, cuda_device, cfg):
    from pipelinerl_amd.finetune.rl import gspo_segment_terms

    batch, _, _ = case("geometry")
    S = int(batch["segment_ids"].max()) + 1
    w = sc.witness(cfg, *columns(batch))
    assert w.sums[2, 0] == 0 and not w.valid[0]                       # the run of segment 0 is empty
    assert (~w.valid).sum() >= (3 if cfg["overlong_filtering"] else 2)  # + the unlabelled one, + overflow = 1 under overlong_filtering
    got = run_all(libprl, cuda_device, batch, cfg)
    assert_checks(f"geometry {_cfg_id(cfg)}", batch, cfg, got, w)
    assert (got[1][~w.valid] == 0).all() and (got[2][~w.valid] == 0).all()
    # n_segments above the largest id: the trailing segments are empty
    w3 = sc.witness(cfg, *columns(batch), n_segments=S + 3)
    got3 = run_all(libprl, cuda_device, batch, cfg, n_seg=S + 3)
    assert_checks(f"geometry {_cfg_id(cfg)} n_segments + 3", batch, cfg, got3, w3)
    assert not got3[0][:, S:].any() and not got3[1][S:].any() and not got3[2][S:].any()
    assert np.array_equal(got3[0][:, :S], got[0]) and np.array_equal(got3[1][:S], got[1]) and np.array_equal(got3[2][:S], got[2])
    assert all(np.array_equal(got3[i], got[i]) for i in (3, 4, 5))
    # the wrapper is the same three launches
    loss, ext_g, ext_c = gspo_segment_terms(_c_cfg(cfg), _pb(batch, cuda_device), torch.from_numpy(batch["new_logprobs"]).to(cuda_device))
    assert np.array_equal(_np(loss), got[3]) and np.array_equal(_np(ext_g), got[4]) and np.array_equal(_np(ext_c), got[5])


@pytest.mark.parametrize("name", ["many", "wide"])
def test_many_segments(libprl, cuda_device, name):
    batch, cfgs, _ = case(name)
    assert (int(batch["segment_ids"].max()) + 1 > 256) and (name != "wide" or batch["labels"].shape[1] > EXPAND_GRID_COLUMNS)
    for cfg in cfgs:
        w = sc.witness(cfg, *columns(batch))
        assert_checks(f"{name} {_cfg_id(cfg)}", batch, cfg, run_all(libprl, cuda_device, batch, cfg), w)


def test_clip_edges(libprl, cuda_device):
    batch, cfgs, _ = case("clip")
    for cfg in cfgs:
        w = sc.witness(cfg, *columns(batch))
        r = w.ratio[1:].reshape(len(RATIOS), 3)
        assert np.allclose(r, np.asarray(RATIOS)[:, None], rtol=1e-6)  # the builder hit its targets
        assert w.indicator[1:].reshape(len(RATIOS), 3).tolist() == [[1.0] * 3, [0.0] * 3, [0.0] * 3, [0.0] * 3, [1.0] * 3]
        c = w.coef[1:].reshape(len(RATIOS), 3)
        # min(r A, clip(r) A) keeps r A below the range for A > 0 and above it for A < 0; the other side is clipped: no gradient
        assert (c[0, 0] != 0 and c[0, 1] == 0 and c[4, 0] == 0 and c[4, 1] != 0 and (c[:, 2] == 0).all() and (c[1:4, :2] != 0).all())
        assert_checks(f"clip {_cfg_id(cfg)}", batch, cfg, run_all(libprl, cuda_device, batch, cfg), w)


def test_exact_tie_on_both_bounds(libprl, cuda_device):
    """epsilon = 0 and new == old: the ratio is exactly 1 = clip_lo = clip_hi.  The clamp changes nothing (indicator 0), min() ties
    and splits the gradient over two equal halves, and the inclusive inside rule keeps both: the full unclipped coefficient."""
    batch, cfgs, _ = case("tie")
    for cfg in cfgs:
        w = sc.witness(cfg, *columns(batch))
        assert (w.lo, w.hi) == (1.0, 1.0) and (w.ratio == 1.0).all() and not w.indicator.any()
        den = np.maximum(w.sums[2], 1e-6)
        assert np.array_equal(w.coef, -np.where(w.valid, w.sums[3], 0.0) * (w.sums[1] / den) * 1.0 / den)  # the full unclipped value
        got = run_all(libprl, cuda_device, batch, cfg)
        assert_checks(f"tie {_cfg_id(cfg)}", batch, cfg, got, w)
        assert not got[2].any() and not got[5].any()


def test_slice_form(libprl, cuda_device):
    """A sequence-parallel slice: ids start at 3, the sums of the WHOLE sequence come from outside (as after the all-reduce),
    grad_scale is the group size; `coef` is indexed by global id, `indicator` by seg - seg[0]."""
    part, cfgs, extra = case("slice")
    for cfg in cfgs:
        whole = sc.witness(cfg, *columns(extra["whole"]))
        own = sc.witness(cfg, *columns(part), n_segments=SLICE_SEGMENTS, guard=False)  # the slice's own sums: part of segment 3, no 0 .. 2
        assert not own.sums[:, :SLICE_FIRST].any()
        w = sc.witness(cfg, *columns(part), n_segments=SLICE_SEGMENTS, sums=whole.sums, grad_scale=extra["grad_scale"])
        assert not np.array_equal(w.ext_c, w.indicator[part["segment_ids"][0]])  # the two indexings differ on this case
        got = run_all(libprl, cuda_device, part, cfg, n_seg=SLICE_SEGMENTS, sums=whole.sums, grad_scale=extra["grad_scale"])
        assert_checks(f"slice {_cfg_id(cfg)}", part, cfg, got, w, sums_witness=own)
        wz = sc.witness(cfg, *columns(part), n_segments=SLICE_SEGMENTS, sums=whole.sums, grad_scale=extra["grad_scale"], zero_out=True)
        gz = run_all(libprl, cuda_device, part, cfg, n_seg=SLICE_SEGMENTS, sums=whole.sums, grad_scale=extra["grad_scale"], zero_out=1)
        assert_checks(f"slice zero_out {_cfg_id(cfg)}", part, cfg, gz, wz, sums_witness=own)
        assert gz[3] == 0 and not gz[1].any() and not gz[4].any()
        assert np.array_equal(gz[2], got[2])  # the statistic's indicator does not depend on zero_out


def test_order_check(libprl, cuda_device):
    """Ids that are not sorted, or leave [0, n_segments) on a labelled token, turn all 4 S sums into NaN; on an unlabelled token
    they do not."""
    batch, cfgs, _ = case("clip")
    cfg = cfgs[0]
    S = int(batch["segment_ids"].max()) + 1
    T = batch["labels"].shape[1]
    c_cfg = _c_cfg(cfg)

    def sums_of(seg_ids=None, labels=None):
        b = dict(batch)
        if seg_ids is not None:
            b["segment_ids"] = seg_ids
        if labels is not None:
            b["labels"] = labels
        out = _np(run_sums(libprl, c_cfg, _dev(b, cuda_device), S))
        torch.cuda.synchronize()
        return out, b

    base, _ = sums_of()
    assert np.isfinite(base).all()
    ids = batch["segment_ids"].copy()
    a, b = np.flatnonzero(ids[0] == 4), np.flatnonzero(ids[0] == 5)
    ids[0, a], ids[0, b[:len(a)]] = 5, 4  # ... 3 5 5 5 4 4 4 5 ...: not non-decreasing
    assert (np.diff(ids[0]) < 0).any()
    assert np.isnan(sums_of(ids)[0]).all(), "unsorted ids"
    assert batch["labels"][0, T - 1] != -100 and batch["labels"][0, 1] != -100
    ids = batch["segment_ids"].copy()
    ids[0, T - 1] = S
    assert np.isnan(sums_of(ids)[0]).all(), "id >= n_segments on a labelled token"
    ids = batch["segment_ids"].copy()
    ids[0, :2] = -1
    assert np.isnan(sums_of(ids)[0]).all(), "negative id on a labelled token"
    ids = batch["segment_ids"].copy()
    labels = batch["labels"].copy()
    ids[0, T - 1], labels[0, T - 1] = S, -100
    got, b = sums_of(ids, labels)
    assert np.isfinite(got).all(), "an out-of-range id on an unlabelled token is not an error"
    mask, terms = sc.token_terms(cfg, *columns(b)[1:])
    want = sc.witness(cfg, *columns(dict(b, segment_ids=np.minimum(ids, S - 1))))  # the token is unlabelled: it enters no sum
    assert mask.sum() == (batch["labels"][0, 1:] != -100).sum() - 1
    assert sc.check_sums(got, want).ok()


def test_non_finite(libprl, cuda_device):
    batch, cfgs, extra = case("nan")
    cfg, s = cfgs[0], extra["nan_segment"]
    w = sc.witness(cfg, *columns(batch))
    assert np.isnan(w.loss) and np.isnan(w.coef[s]) and np.isfinite(np.delete(w.coef, s)).all()
    sums, coef, ind, loss, ext_g, ext_c = run_all(libprl, cuda_device, batch, cfg)
    rt = sc.check_terms(coef, ind, loss, w)  # NaN where the witness is NaN, the metric everywhere else
    print(f"nan: coef {rt.coef_err:.3e} (bound {sc.COEF_BOUND:.1e})")
    assert np.isnan(loss) and np.isnan(coef[s]) and rt.ok(), str(rt)
    keep = np.arange(sums.shape[1]) != s
    clean = dataclasses.replace(w, sums=w.sums[:, keep], abs_sums=w.abs_sums[:, keep])
    assert sc.check_sums(sums[:, keep], clean).ok() and np.isnan(sums[0, s])
    assert sc.check_tokens(ext_g, ext_c, batch["segment_ids"], coef, ind)[0] == 0


def test_k2_under_gspo(libprl, cuda_device):
    """K2+K3 with the sequence-level columns: aligned (vector kernel, T % 4 tails) and 4 / 8 bytes off 16-byte alignment (the scalar
    kernel).  `g_nlp` is `ext_g` on the labelled columns >= 1 and 0 elsewhere, bit for bit; there is no entropy gradient."""
    from pipelinerl_amd._lib import STAT_INDEX
    from pipelinerl_amd.finetune.rl import gspo_segment_terms, grpo_loss_from_logprobs

    full, _, _ = case("geometry")
    cfg = loss_cfg(entropy_bonus=0.01, final_entropy_bonus=0.01)  # an entropy coefficient, so that g_ent is delivered at all
    c_cfg = _c_cfg(cfg)
    assert c_cfg.use_entropy_loss == 1
    T = full["labels"].shape[1]
    for cut in (T, T - 1, T - 2, T - 3):
        b = {k: (np.ascontiguousarray(v[:, :cut]) if isinstance(v, np.ndarray) else v) for k, v in full.items()}
        want = orl.token_loss(b, b["new_logprobs"][:, 1:], b["entropy"][:, 1:], cfg, 0, 10, True)
        labelled = b["labels"][0] != -100
        labelled[0] = False
        pb = _pb(b, cuda_device)
        _, ext_g, ext_c = gspo_segment_terms(c_cfg, pb, torch.from_numpy(b["new_logprobs"]).to(cuda_device))
        xg, xc = _np(ext_g), _np(ext_c)
        for misalign in (False, True):
            def dev(a, dtype):
                t = torch.from_numpy(np.ascontiguousarray(a)).to(cuda_device).to(dtype)
                if misalign:  # place the data 4 bytes (fp32) / 8 bytes (i64) off 16-byte alignment
                    buf = torch.empty(t.numel() + 1, dtype=dtype, device=cuda_device)
                    buf[1:] = t.reshape(-1)
                    return buf[1:].view_as(t)
                return t
            batch = _pb(b, cuda_device)
            for k in ("labels", "position_ids"):
                setattr(batch, k, dev(b[k], torch.long))
            for k in ("old_logprobs", "ref_logprobs", "advantages", "rewards", "group_tokens", "num_labels", "overflow"):
                setattr(batch, k, dev(b[k], torch.float32))
            assert (batch.labels.data_ptr() % 16 != 0) == misalign
            loss, stats, g_nlp, g_ent = grpo_loss_from_logprobs(c_cfg, batch, dev(b["new_logprobs"], torch.float32), dev(b["entropy"], torch.float32),
                                                                ext_token_grad=dev(xg, torch.float32), ext_clamp_indicator=dev(xc, torch.float32))
            g, s = _np(g_nlp), _np(stats)
            label = f"cut {cut} misalign {misalign}"
            assert np.array_equal(g.view(np.uint32)[0, labelled], xg.view(np.uint32)[0, labelled]), label
            assert not g[0, ~labelled].any(), label
            assert g_ent is not None and not _np(g_ent).any(), label
            assert s[STAT_INDEX["loss"]] == 0 and loss.item() == 0, label  # the token kernel adds nothing to the GSPO loss
            clamp = float((xc[0, labelled].astype(np.float64) / b["num_labels"][0, labelled]).sum())
            got_clamp = s[STAT_INDEX["clamp_log_ratio_new_old_indicator"]]
            assert abs(got_clamp - clamp) <= FP_TOL * max(abs(clamp), 1.0), (label, got_clamp, clamp)
            worst = 0.0
            for k, i in STAT_INDEX.items():
                if k in ("loss", "clamp_log_ratio_new_old_indicator"):
                    continue
                wv = float(want["num_sequences"]) if k == "num_sequences" else (0.0 if k.startswith(("nonfinite", "bad_")) else float(want["stats"][k]))
                worst = max(worst, abs(s[i] - wv) / max(abs(wv), 1.0))
                assert abs(s[i] - wv) <= FP_TOL * max(abs(wv), 1.0), (label, k, s[i], wv)
            print(f"K2 under GSPO {label}: clamp statistic {got_clamp:.6f} vs {clamp:.6f}; other statistics {worst:.2e} (tolerance {FP_TOL:.0e})")


def test_reproducible(libprl, cuda_device):
    batch, cfgs, _ = case("geometry")
    runs = [run_all(libprl, cuda_device, batch, cfgs[3]) for _ in range(4)]
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert np.array_equal(a.view(np.uint64 if a.dtype == np.float64 else np.uint32), b.view(np.uint64 if b.dtype == np.float64 else np.uint32))


class FakeModel(torch.nn.Module):
    def __init__(self, logits):
        super().__init__()
        self.logits = torch.nn.Parameter(logits)

    def forward(self, **kwargs):
        return types.SimpleNamespace(logits=self.logits)


def _kernel_token_grads(c_cfg, pb, nlp, ent):
    """(loss, g_nlp [1, T] numpy) of the sequence-level path on given log-probs - the kernels the tests above hold to the witness."""
    from pipelinerl_amd.finetune.rl import gspo_segment_terms, grpo_loss_from_logprobs

    loss, ext_g, ext_c = gspo_segment_terms(c_cfg, pb, nlp)
    _, _, g_nlp, _ = grpo_loss_from_logprobs(c_cfg, pb, nlp, ent, ext_token_grad=ext_g, ext_clamp_indicator=ext_c)
    return loss, _np(g_nlp)


def test_end_to_end_rl_step(libprl, cuda_device):
    """`rl_step` on the head of the run-geometry case (2048 tokens, V = 1031): the loss under the loss metric (the witness on
    K1's own log-probs), d logits entry by entry with the token gradients of the kernels checked above."""
    from pipelinerl_amd.finetune.rl import RLConfig, logprob_entropy, rl_step

    batch, cfgs, extra = case("e2e")
    cfg = cfgs[0]
    pb = _pb(batch, cuda_device)
    model = FakeModel(torch.from_numpy(extra["logits"]).to(cuda_device))
    loss, stats = rl_step(model, pb, 0, 10, RLConfig(**cfg))
    loss.backward()
    nlp, ent, _, _ = logprob_entropy(model.logits.detach(), pb.input_ids, 1.0)
    fwd = float(np.abs(_np(nlp)[0, 1:] - batch["new_logprobs"][0, 1:]).max())
    print(f"e2e rl_step: K1 log-probs vs fp64 {fwd:.3e} nats (bound {gc.FWD_BOUND['k1_random_g']:.1e})")
    assert fwd <= gc.FWD_BOUND["k1_random_g"]
    w = sc.witness(cfg, *columns(dict(batch, new_logprobs=_np(nlp))))
    err = abs(loss.item() - w.loss) / w.loss_scale
    print(f"e2e rl_step: loss {loss.item():.9e} want {w.loss:.9e}, error {err:.3e} (bound {sc.LOSS_BOUND:.1e})")
    assert err <= sc.LOSS_BOUND
    assert stats["loss"] == loss.item()
    k_loss, g_nlp = _kernel_token_grads(_c_cfg(cfg), pb, nlp, ent)
    assert k_loss.item() == loss.item()
    rt = sc.check_terms(*run_all(libprl, cuda_device, dict(batch, new_logprobs=_np(nlp)), cfg)[1:4], w)
    assert rt.ok(), str(rt)
    rid, g, gh = gc.token_rows(batch["input_ids"], g_nlp[:, 1:], np.zeros_like(g_nlp[:, 1:]))
    assert np.count_nonzero(g) > 1000
    res = gc.dlogits_error(_np(model.logits.grad)[0], extra["logits"][0], rid, g, gh, 1.0)
    print(f"e2e rl_step: d logits per entry {res.err:.3e} (bound {gc.DLOGITS_BOUND['k1_random_g']:.1e})")
    assert res.ok(gc.DLOGITS_BOUND["k1_random_g"]), str(res)


def test_end_to_end_fused_head(libprl, cuda_device):
    """`rl_step_fused_head` on the same tokens with H = 128 (the head needs whole 64-wide vocabulary tiles: V = 1088): its loss
    equals `rl_step`'s on the same model, d hidden and d W pass the head's per-entry check."""
    import copy

    import head_grad_checks as hg
    from pipelinerl_amd.finetune.rl import RLConfig, rl_step
    from pipelinerl_amd.fused_head import rl_step_fused_head
    from test_gpu_lmhead_fused import _own_logprobs, _per_entry

    T, H, V = E2E_T, 128, 1088
    g = torch.Generator().manual_seed(109)
    hidden = torch.randn(1, T, H, generator=g).to(torch.bfloat16)
    W = torch.randn(V, H, generator=g) * (2.0 / H ** 0.5)
    ids = build(e2e_segments(), 109, vocab=V)["input_ids"]
    nlp64, _, _ = gc.forward_witness(hg.logits64(hidden[0], W)[:-1], ids[0, 1:], 1.0)
    batch = build(e2e_segments(), 109, vocab=V, new=np.concatenate([[0.0], nlp64]).astype(F32))
    assert np.array_equal(batch["input_ids"], ids)
    cfg = loss_cfg()

    class Body(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.h = torch.nn.Parameter(hidden.float())

        def forward(self, **kw):
            return (self.h.to(torch.bfloat16),)

    class LM(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.model = Body()
            self.lm_head = torch.nn.Linear(H, V, bias=False)
            with torch.no_grad():
                self.lm_head.weight.copy_(W)

        def forward(self, **kw):
            return types.SimpleNamespace(logits=self.model(**kw)[0].float() @ self.lm_head.weight.t())

    a = LM().to(cuda_device)
    b = copy.deepcopy(a)
    pb = _pb(batch, cuda_device)
    la, _ = rl_step(a, pb, 0, 10, RLConfig(**cfg))
    lb, _ = rl_step_fused_head(b, pb, 0, 10, RLConfig(**cfg))
    lb.backward()
    torch.cuda.synchronize()
    print(f"e2e fused head: loss {lb.item():.9e}, rl_step {la.item():.9e}")
    assert abs(la.item() - lb.item()) <= FP_TOL * abs(la.item())
    hd, Wd = hidden.to(cuda_device), b.lm_head.weight.detach()
    nlp, ent = _own_logprobs(hd, Wd, pb, 1.0)
    w = sc.witness(cfg, *columns(dict(batch, new_logprobs=_np(nlp))))
    err = abs(lb.item() - w.loss) / w.loss_scale
    print(f"e2e fused head: loss error {err:.3e} (bound {sc.LOSS_BOUND:.1e})")
    assert err <= sc.LOSS_BOUND
    _, g_nlp = _kernel_token_grads(_c_cfg(cfg), pb, nlp, ent)
    _per_entry(hd, Wd, batch["input_ids"], g_nlp, None, 1.0, gh=b.model.h.grad.to(torch.bfloat16), gw=b.lm_head.weight.grad,
               label="e2e fused head")
