"""The logits kernels at the edges of their own regions, on padded rows, on more rows than one wave of workgroups and
on rows as a trained model makes them - through the C ABI, every fused variant and the default dispatch, fp32 and bf16,
out of place and in place.

Log-prob, entropy and lse2 are compared with fp64 (`grad_checks.forward_witness`), d logits per entry with
`grad_checks.dlogits_error`; every bound is 4 x the error of the reference's own fp32 arithmetic on the same family of
inputs (`grad_checks.DLOGITS_BOUND` / `FWD_BOUND`, re-measured on the CPU by tests/test_grad_checks_host.py).

Paths no other test reaches, and the case that reaches each:
  * the scalar tail of the row-resident kernel (both passes): V = 152 067 with row stride 152 068  (test_region_edges)
  * row-resident with an empty streamed part (V = 102 400), with the vector tail only (102 404), with exactly one full
    tile and no tail (102 400 + 8192) and with one tile + one vector (+ 4)                         (test_region_edges)
  * the scalar tail after a vector body in the two-sweep kernels: V = 4099, stride 4104            (test_region_edges)
  * a row stride different from the vocabulary, aligned and unaligned, sentinel-filled padding    (test_padded_row_stride)
  * rows x cols = 3 x 17 at full vocabulary                                                        (test_rows_by_cols_geometry)
  * a grid of more than one workgroup per CU: 775 rows x 102 400 and 5000 rows x 4099              (test_more_rows_than_one_wave)
"""

import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import rl_loss as orl

import grad_checks as gc

pytestmark = pytest.mark.gpu

# ---- the one table of launch constants -----------------------------------------------------------------------------
# PRL_FUSED_VARIANT -> kernel name as `prl_last_fused_kernel()` reports it ({T} = F32 / BF16).  The region layout of a
# kernel (register head, LDS head, full tiles, vector tail, scalar tail) is derived from the template arguments in that
# name by grad_checks.kernel_regions: a rewrite that changes a launch shape changes this table and nothing else.
FUSED = {
    0: "fused_logits_loss_kernel<{T},256,4,false,false>",
    4: "fused_logits_loss_kernel<{T},512,4,true,true>",
    6: "fused_logits_loss_kernel<{T},1024,4,true,true>",
    21: "fused_logits_loss_keep_kernel<{T},1024,2,16,9,true>",
}
DEFAULT_VARIANT = {"f32": 21, "bf16": 4}
K1 = {"fwd": (256, 8), "bwd": (256, 4)}  # logprob_entropy_{fwd,bwd}_kernel: (BLOCK, UNROLL)
TNAME = {"f32": "F32", "bf16": "BF16"}
ESZ = {"f32": 4, "bf16": 2}
SENTINEL = 12288.0  # exact in bf16; as a logit it would own the softmax, as a gradient it cannot be mistaken

LOSS = {
    # kl > 0 and an entropy bonus: every labelled row has g != 0 and gH != 0
    "kl_ent": dict(policy_loss="ppo", epsilon_low=0.2, epsilon_high=0.2, kl_coef=0.05, final_kl_coef=0.05, entropy_bonus=0.01,
                   final_entropy_bonus=0.01, batch_size=8, clamp_log_ratio_ref_new_value=5, divide_advantage_by_std=False),
    # the BASELINE loss: PPO-clipped rows have an exactly zero gradient
    "grpo_clip": dict(policy_loss="ppo", epsilon_low=0.02, epsilon_high=0.02, kl_coef=0.0, final_kl_coef=0.0, batch_size=64,
                      clamp_log_ratio_ref_new_value=5, divide_advantage_by_std=False),
}


def vec_ok(dtype: str, stride: int) -> bool:
    return (stride * ESZ[dtype]) % 16 == 0


def expected_kernel(variant, dtype: str, vocab: int, stride: int) -> str:
    v = DEFAULT_VARIANT[dtype] if variant is None else variant
    k = gc.parse_kernel(FUSED[v].format(T=TNAME[dtype]))
    if k["kreg"] + k["klds"] and (not vec_ok(dtype, stride) or vocab // k["nv"] < (k["kreg"] + k["klds"]) * k["block"]):
        v = 6  # rows too short or unaligned for the row-resident shape
    return FUSED[v].format(T=TNAME[dtype])


def all_regions(dtype: str, vocab: int, stride: int):
    """Region lists of every kernel a (dtype, vocab, stride) row can meet: the four fused variants and K1 fwd / bwd."""
    out = {}
    for v in FUSED:
        name = expected_kernel(v, dtype, vocab, stride)
        out[name] = gc.regions_of_kernel(name, vocab, vec_ok(dtype, stride))
    nv = 16 // ESZ[dtype]
    for k, (block, unroll) in K1.items():
        out[k] = gc.kernel_regions(vocab, nv, block, unroll, vec_ok=vec_ok(dtype, stride))
    return out


def edge_columns(dtype: str, vocab: int, stride: int):
    """(first and last column of every region of every kernel, the boundaries between two regions)."""
    cols, bounds = set(), set()
    for regs in all_regions(dtype, vocab, stride).values():
        for _, lo, hi in regs:
            cols.update((lo, hi - 1))
            if lo > 0:
                bounds.add(lo)
    return sorted(cols), sorted(bounds)


# ---- inputs (pure host code; tests/test_grad_checks_host.py measures the reference on the same arrays) ---------------
def _randn(rows: int, vocab: int, seed: int) -> np.ndarray:
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, vocab, generator=g) * 2).numpy()


def edge_rows(dtype: str, vocab: int, stride: int):
    """logits [R, V] and labels [R]: for every edge column one row with the label there and one with the row maximum
    there (10 above everything else); for every region boundary one row with two equal maxima on either side."""
    cols, bounds = edge_columns(dtype, vocab, stride)
    R = 2 * len(cols) + len(bounds)
    x = _randn(R, vocab, vocab + stride)
    rng = np.random.default_rng(vocab)
    labels = rng.integers(0, vocab, size=R)
    top = np.abs(x).max() + 10.0
    for i, c in enumerate(cols):
        labels[2 * i] = c
        x[2 * i + 1, c] = top
    for i, b in enumerate(bounds):
        x[2 * len(cols) + i, b - 1:b + 1] = top
    return x, labels


def trained_rows(vocab: int, offset_1000: bool):
    """Rows as a trained model makes them.  `offset_1000`: only the two rows with a common offset of +-1000 (a family of
    its own: an fp32 logsumexp near 1000 carries 3e-5 of rounding whatever the arithmetic)."""
    if offset_1000:
        x = _randn(2, vocab, vocab + 1000)
        x[0] += 1000.0
        x[1] -= 1000.0
        return x, np.array([5, vocab - 1])
    x = _randn(6, vocab, vocab + 5)
    rng = np.random.default_rng(vocab + 5)
    labels = rng.integers(0, vocab, size=6)
    x[0, labels[0]] = x[0].max() + 20.0   # p(label) ~ 1: 1 - p cancels
    x[1] += 30.0
    x[2] -= 30.0
    x[3] = 1.5                            # uniform: entropy ln V
    x[4, rng.choice(vocab, size=min(1000, vocab // 2), replace=False)] = -1e4
    labels[4] = int(np.argmax(x[4]))
    return x, labels                      # row 5: plain 2 * randn


@functools.lru_cache(maxsize=4)
def build_case(kind: str, dtype: str, vocab: int, stride: int, loss: str = "kl_ent", temperature: float = 0.7,
               rows: int = 0, seqs: int = 1):
    """One batch of `seqs` sequences over the rows of `kind` (+ one last row per sequence that predicts nothing), the
    oracle's token gradients for it and the fp64 forward witness.  Everything on the host."""
    if kind == "edges":
        x, labels = edge_rows(dtype, vocab, stride)
    elif kind in ("trained", "offset_1000"):
        x, labels = trained_rows(vocab, kind == "offset_1000")
    else:  # "randn": `rows` rows of 2 * randn
        x = _randn(rows, vocab, vocab + rows)
        labels = np.random.default_rng(rows).integers(0, vocab, size=rows)
    if dtype == "bf16":
        x = gc.round_bf16(x)
    R = x.shape[0]
    assert R % seqs == 0
    per = R // seqs
    L = per + 1
    rng = np.random.default_rng(R + vocab)
    logits = np.concatenate([x.reshape(seqs, per, vocab), _randn(seqs, vocab, 3).reshape(seqs, 1, vocab)], axis=1)
    if dtype == "bf16":
        logits = gc.round_bf16(logits)
    ids = np.concatenate([rng.integers(0, vocab, size=(seqs, 1)), labels.reshape(seqs, per)], axis=1).astype(np.int64)
    nlp64, ent64, lse64 = gc.forward_witness(logits[:, :-1].reshape(R, vocab), labels, temperature)
    lab = ids.copy()
    lab[:, 0] = -100
    unl = rng.random((seqs, L)) < 0.12           # unlabelled tokens scattered through the range
    unl[:, 1:3] = False
    lab[unl] = -100
    old = nlp64.reshape(seqs, per) + rng.uniform(-0.005, 0.005, (seqs, per))  # ratio well inside both clip ranges
    adv = rng.normal(0, 1, (seqs, per))
    clip = rng.random((seqs, per)) < 0.15        # ratio far outside, on the side where PPO clips
    up = rng.random((seqs, per)) < 0.5
    old = np.where(clip, nlp64.reshape(seqs, per) - np.where(up, 0.5, -0.5), old)
    adv = np.where(clip, np.where(up, np.abs(adv) + 0.1, -np.abs(adv) - 0.1), adv)
    ref = old + rng.normal(0, 0.05, (seqs, per))
    pad = lambda a: np.concatenate([np.zeros((seqs, 1)), a], axis=1).astype(np.float32)  # noqa: E731
    batch = {
        "input_ids": ids, "labels": lab, "old_logprobs": pad(old), "ref_logprobs": pad(ref), "advantages": pad(adv),
        "rewards": pad(rng.integers(0, 2, (seqs, per))), "group_tokens": np.full((seqs, L), 37.0, np.float32),
        "num_labels": np.full((seqs, L), float((lab != -100).sum()), np.float32), "overflow": np.zeros((seqs, L), np.float32),
    }
    tok = orl.token_loss(batch, nlp64.reshape(seqs, per).astype(np.float32), ent64.reshape(seqs, per).astype(np.float32),
                         LOSS[loss], 2, 10, False)
    row_ids, g, gh = gc.token_rows(ids, tok["g_nlp"], tok["g_ent"])
    fwd = tuple(np.concatenate([np.zeros((seqs, 1)), a.reshape(seqs, per)], axis=1) for a in (nlp64, ent64, lse64))
    return dict(logits=logits, batch=batch, row_ids=row_ids, g=g, gh=gh, fwd=fwd, seqs=seqs, L=L, vocab=vocab,
                temperature=temperature, loss=loss)


# ---- device side -----------------------------------------------------------------------------------------------------
def _strided(a: np.ndarray, stride: int, tdtype, dev, fill=SENTINEL):
    """[N, stride] device buffer holding the rows of `a` [N, V] and `fill` in the padding."""
    n, v = a.shape
    buf = torch.full((n, stride), fill, dtype=tdtype, device=dev)
    buf[:, :v] = torch.from_numpy(a).to(dev).to(tdtype)
    return buf


def launch_fused(lib, dev, case, dtype, stride, inplace):
    from pipelinerl_amd import _lib
    from pipelinerl_amd.finetune.rl import RLConfig, make_loss_config

    c_cfg, _, _ = make_loss_config(RLConfig(**LOSS[case["loss"]], temperature=case["temperature"]), 2, 10)
    S, L, V = case["seqs"], case["L"], case["vocab"]
    td = torch.float32 if dtype == "f32" else torch.bfloat16
    src = _strided(case["logits"].reshape(S * L, V), stride, td, dev)
    grad = src if inplace else torch.full_like(src, SENTINEL)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in case["batch"].items()}
    nlp, ent, lse2 = (torch.full((S, L), 7.0, device=dev) for _ in range(3))
    _lib.check(lib.prl_fused_logits_loss(
        ctypes.byref(c_cfg), S, L, V, src.data_ptr(), 0 if dtype == "f32" else 1, stride, case["temperature"],
        d["input_ids"].data_ptr(), d["labels"].data_ptr(), d["old_logprobs"].data_ptr(), d["ref_logprobs"].data_ptr(),
        d["advantages"].data_ptr(), d["rewards"].data_ptr(), d["group_tokens"].data_ptr(), d["overflow"].data_ptr(),
        nlp.data_ptr(), ent.data_ptr(), lse2.data_ptr(), grad.data_ptr(), _lib.current_stream_ptr(dev)))
    torch.cuda.synchronize()
    kernel = lib.prl_last_fused_kernel().decode()
    out = (nlp.cpu().numpy(), ent.cpu().numpy(), lse2.cpu().numpy(), grad.float().cpu().numpy())
    del src, grad, d
    return out, kernel


def check_forward(nlp, ent, lse2, case, family, rows=None):
    """Token-aligned kernel outputs against fp64: column 0 is 0, the rest within the family's bound (nats)."""
    w_nlp, w_ent, w_lse = case["fwd"]
    assert not nlp[:, 0].any() and not ent[:, 0].any() and not lse2[:, 0].any(), "column 0 has no prediction"
    tol = gc.FWD_BOUND[family]
    for name, got, want in (("new_logprobs", nlp, w_nlp), ("entropy", ent, w_ent), ("lse2 * ln 2", lse2 * np.log(2.0), w_lse)):
        err = np.abs(got[:, 1:].astype(np.float64) - want[:, 1:])
        worst = np.unravel_index(int(np.argmax(err)), err.shape)
        print(f"[fwd] {family} {name}: max abs err {err.max():.3e} (bound {tol:.1e})")
        assert err.max() <= tol, f"{name}: |err| {err.max():.3e} > {tol:.1e} at (seq, token) {worst}"


def token_grads(case, nlp, ent):
    """Row-level (g, gH) the oracle's token loss gives for the kernel's OWN log-probs and entropies.  The fused kernel
    derives them from its fp32 log-prob; where the policy and the KL gradient nearly cancel, g is ill-conditioned in
    that log-prob (3e-7 nats moved one g of 5e-4 by 1e-5 relative), which is the token loss's conditioning and not the
    row kernel's error.  The log-probs and entropies themselves are held to fp64 by `check_forward`."""
    tok = orl.token_loss(case["batch"], nlp[:, 1:], ent[:, 1:], LOSS[case["loss"]], 2, 10, False)
    _, g, gh = gc.token_rows(case["batch"]["input_ids"], tok["g_nlp"], tok["g_ent"])
    assert np.array_equal(g == 0, case["g"] == 0) and np.array_equal(gh == 0, case["gh"] == 0), "clip / mask decisions differ"
    return g, gh


def check_grad(grad, case, dtype, stride, kernel, family, rows=None, g_gh=None):
    """d logits per entry (all rows, or the listed ones), padding columns still SENTINEL."""
    V = case["vocab"]
    flat = case["logits"].reshape(-1, V)
    sel = np.arange(flat.shape[0]) if rows is None else np.asarray(rows)
    if stride > V:
        assert (grad[:, V:] == SENTINEL).all(), "padding columns of grad_logits were written"
    g, gh = g_gh if g_gh is not None else (case["g"], case["gh"])
    res = gc.dlogits_error(grad[sel, :V], flat[sel], case["row_ids"][sel], g[sel], gh[sel], case["temperature"],
                           out_rounding=gc.BF16_ROUNDING if dtype == "bf16" else 0.0,
                           regions=gc.regions_of_kernel(kernel, V, vec_ok(dtype, stride)))
    print(f"[dlogits] {family} V={V} stride={stride} {dtype} {kernel}: {res.err:.3e} (bound {gc.DLOGITS_BOUND[family]:.1e})")
    assert res.ok(gc.DLOGITS_BOUND[family]), f"{kernel} V={V} stride={stride}: {res}"
    return res


def run_variants(lib, dev, monkeypatch, case, dtype, stride, family, variants, rows=None):
    V = case["vocab"]
    for variant in variants:
        if variant is None:
            monkeypatch.delenv("PRL_FUSED_VARIANT", raising=False)
        else:
            monkeypatch.setenv("PRL_FUSED_VARIANT", str(variant))
        for inplace in (False, True):
            (nlp, ent, lse2, grad), kernel = launch_fused(lib, dev, case, dtype, stride, inplace)
            print(f"[kernel] {family} V={V} stride={stride} {dtype} variant={variant} inplace={inplace}: {kernel}")
            assert kernel == expected_kernel(variant, dtype, V, stride), kernel
            check_forward(nlp, ent, lse2, case, family)
            check_grad(grad, case, dtype, stride, kernel, family, rows, token_grads(case, nlp, ent))
    torch.cuda.empty_cache()


def _tile(variant: int, dtype: str) -> int:
    k = gc.parse_kernel(FUSED[variant].format(T=TNAME[dtype]))
    return k["block"] * k["unroll"] * k["nv"]


# 1. region edges -----------------------------------------------------------------------------------------------------
HEAD = 102400  # (16 + 9) x 1024 vectors x 4 fp32 columns: the dispatch threshold of the row-resident kernel
KEEP_SIZES = [(HEAD, HEAD), (HEAD + 4, HEAD + 4), (HEAD + 8192, HEAD + 8192), (HEAD + 8192 + 4, HEAD + 8192 + 4),
              (151936, 151936), (152064, 152064), (152067, 152068)]


@pytest.mark.parametrize("vocab,stride", KEEP_SIZES)
def test_region_edges_row_resident(libprl, cuda_device, monkeypatch, vocab, stride):
    """Variant 21 fp32 (and the default dispatch): label, maximum and tied maxima at the first and last column of the
    register head, the LDS head, the streamed tiles, the vector tail and the scalar tail."""
    assert gc.parse_kernel(FUSED[21].format(T="F32"))["block"] * 25 * 4 == HEAD
    case = build_case("edges", "f32", vocab, stride)
    assert "keep_kernel" in expected_kernel(21, "f32", vocab, stride)
    run_variants(libprl, cuda_device, monkeypatch, case, "f32", stride, "edges", [21, None])


def _two_sweep_sizes():
    out = []
    for dtype in ("f32", "bf16"):
        nv = 16 // ESZ[dtype]
        sizes = {(4099, 4099), (4099, 4104)}  # an odd vocabulary: dense (all scalar) and with an aligned padded stride
        for v in (0, 4, 6):
            t = _tile(v, dtype)
            sizes.update({(t - nv, t - nv), (t, t), (t + nv, t + nv)})
        out += [(dtype, v, s) for v, s in sorted(sizes)]
    return out


@pytest.mark.parametrize("dtype,vocab,stride", _two_sweep_sizes())
def test_region_edges_two_sweep(libprl, cuda_device, monkeypatch, dtype, vocab, stride):
    """Every variant on rows one vector below, at and above one full tile of each two-sweep shape, and on an odd
    vocabulary with and without an aligned padded stride (vector body + scalar tail / scalar everywhere)."""
    case = build_case("edges", dtype, vocab, stride)
    run_variants(libprl, cuda_device, monkeypatch, case, dtype, stride, "edges", [0, 4, 6, 21, None])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_region_edges_k1(libprl, cuda_device, dtype):
    """prl_logprob_entropy_fwd / _bwd on the edge rows: V = 152 067 with an aligned stride (tiles, vector tail and
    scalar tail) and dense (scalar everywhere), in place and out of place."""
    from pipelinerl_amd import _lib

    for vocab, stride in ((152067, 152072), (4099, 4099)):
        case = build_case("edges", dtype, vocab, stride)
        S, L, V, temp = case["seqs"], case["L"], vocab, case["temperature"]
        td = torch.float32 if dtype == "f32" else torch.bfloat16
        code = 0 if dtype == "f32" else 1
        ids = torch.from_numpy(case["batch"]["input_ids"]).to(cuda_device)
        # token-aligned upstream gradients: the oracle's, so that the witness is the fused one
        g = torch.zeros(S, L, device=cuda_device)
        gh = torch.zeros(S, L, device=cuda_device)
        g[:, 1:] = torch.from_numpy(case["g"].reshape(S, L)[:, :-1]).float().to(cuda_device)
        gh[:, 1:] = torch.from_numpy(case["gh"].reshape(S, L)[:, :-1]).float().to(cuda_device)
        for inplace in (False, True):
            src = _strided(case["logits"].reshape(S * L, V), stride, td, cuda_device)
            nlp, ent, lse2 = (torch.full((S, L), 7.0, device=cuda_device) for _ in range(3))
            _lib.check(libprl.prl_logprob_entropy_fwd(S, L, V, src.data_ptr(), code, stride, ids.data_ptr(), temp, nlp.data_ptr(),
                                                      ent.data_ptr(), lse2.data_ptr(), _lib.current_stream_ptr(cuda_device)))
            grad = src if inplace else torch.full_like(src, SENTINEL)
            _lib.check(libprl.prl_logprob_entropy_bwd(S, L, V, src.data_ptr(), code, stride, ids.data_ptr(), temp, lse2.data_ptr(),
                                                      ent.data_ptr(), g.data_ptr(), gh.data_ptr(), None, grad.data_ptr(),
                                                      _lib.current_stream_ptr(cuda_device)))
            torch.cuda.synchronize()
            check_forward(nlp.cpu().numpy(), ent.cpu().numpy(), lse2.cpu().numpy(), case, "edges")
            block, unroll = K1["bwd"]
            name = f"fused_logits_loss_kernel<{TNAME[dtype]},{block},{unroll},false,false>"  # same row walk as K1 backward
            check_grad(grad.float().cpu().numpy(), case, dtype, stride, name, "edges")
            del src, grad
    torch.cuda.empty_cache()


# 2. padded row stride ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,pad", [("f32", 4), ("f32", 61), ("bf16", 8), ("bf16", 4), ("bf16", 61)])
def test_padded_row_stride(libprl, cuda_device, monkeypatch, dtype, pad):
    """logits_row_stride = vocab + pad, padding of the logits and of the gradient buffer filled with a sentinel: the
    answers are those of the dense rows and the padding is never written.  An unaligned stride takes the two-sweep
    kernel (scalar path)."""
    for vocab in (152064, 4100):
        case = build_case("randn", dtype, vocab, vocab, rows=6)
        stride = vocab + pad
        monkeypatch.delenv("PRL_FUSED_VARIANT", raising=False)
        dense, k_dense = launch_fused(libprl, cuda_device, case, dtype, vocab, False)
        for variant in (None, 0, 21):
            if variant is None:
                monkeypatch.delenv("PRL_FUSED_VARIANT", raising=False)
            else:
                monkeypatch.setenv("PRL_FUSED_VARIANT", str(variant))
            for inplace in (False, True):
                out, kernel = launch_fused(libprl, cuda_device, case, dtype, stride, inplace)
                print(f"[kernel] padded V={vocab} stride={stride} {dtype} variant={variant} inplace={inplace}: {kernel}")
                assert kernel == expected_kernel(variant, dtype, vocab, stride), kernel
                if not vec_ok(dtype, stride):
                    assert kernel.startswith("fused_logits_loss_kernel<"), kernel
                check_forward(*out[:3], case, "randn")
                check_grad(out[3], case, dtype, stride, kernel, "randn", g_gh=token_grads(case, out[0], out[1]))
                if kernel == k_dense and vec_ok(dtype, stride) == vec_ok(dtype, vocab):  # same kernel, same walk: not a bit may change
                    for a, b in zip(out[:3], dense[:3]):
                        assert np.array_equal(a, b)
                    assert np.array_equal(out[3][:, :vocab], dense[3])
    torch.cuda.empty_cache()


# 3. rows x cols ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_rows_by_cols_geometry(libprl, cuda_device, monkeypatch, dtype):
    """rows = 3, cols = 17 at V = 152 064 (padded layout): column 0 outputs are 0, each sequence's last logits row gets
    a zero gradient, no row uses its neighbour's label (every row's label entry is checked per entry)."""
    case = build_case("randn", dtype, 152064, 152064, rows=48, seqs=3)
    assert case["L"] == 17
    run_variants(libprl, cuda_device, monkeypatch, case, dtype, 152064, "randn", [None, 0])
    (_, _, _, grad), _ = launch_fused(libprl, cuda_device, case, dtype, 152064, True)
    for s in range(3):
        assert not grad[s * 17 + 16].any(), "the last logits row of a sequence predicts nothing"


# 4. more rows than one wave of workgroups ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,vocab,rows,variants", [("f32", HEAD, 3 * 256 + 7, [21]), ("f32", 4099, 5000, [0, 4, 6]),
                                                       ("bf16", 4099, 5000, [4])])
def test_more_rows_than_one_wave(libprl, cuda_device, monkeypatch, dtype, vocab, rows, variants):
    """The grid exceeds one workgroup per CU (256 CUs) several times over; unlabelled and PPO-clipped rows (exactly zero
    gradient under the BASELINE loss) are scattered between computed ones.  Log-prob / entropy / lse2 for every row;
    d logits per entry on the first, the last and a seeded sample of 48 rows, and exact zeros on every zero row."""
    case = build_case("randn", dtype, vocab, vocab, loss="grpo_clip", temperature=1.0, rows=rows)
    zero = np.flatnonzero((case["g"] == 0) & (case["gh"] == 0))
    live = np.flatnonzero(case["g"] != 0)
    assert len(zero) > rows // 8 and len(live) > rows // 2 and np.any(np.diff(zero) > 1)
    sample = np.unique(np.concatenate([[0, rows - 1, rows], np.random.default_rng(rows).choice(rows, 48, replace=False)]))
    for variant in variants:
        monkeypatch.setenv("PRL_FUSED_VARIANT", str(variant))
        for inplace in (False, True):
            (nlp, ent, lse2, grad), kernel = launch_fused(libprl, cuda_device, case, dtype, vocab, inplace)
            print(f"[kernel] many rows V={vocab} rows={rows} {dtype} variant={variant} inplace={inplace}: {kernel}")
            assert kernel == expected_kernel(variant, dtype, vocab, vocab), kernel
            check_forward(nlp, ent, lse2, case, "randn")
            check_grad(grad, case, dtype, vocab, kernel, "randn", rows=sample, g_gh=token_grads(case, nlp, ent))
            assert not grad[zero].any(), "unlabelled / clipped / last rows must be exactly zero"
            assert np.abs(grad[live]).max(axis=1).min() > 0, "every labelled, unclipped row carries a gradient"
            del grad
    torch.cuda.empty_cache()


# 5. rows as a trained model makes them ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("vocab", [152064, 4099])
def test_trained_model_rows(libprl, cuda_device, monkeypatch, dtype, vocab):
    """p(label) ~ 1, a common offset of +-30, a uniform row, 1000 entries at -1e4, at temperature 0.3, 0.7 and 2.0; a
    common offset of +-1000 at temperature 1 (its own family and bound)."""
    variants = [None, 0, 21] if vocab > HEAD else [None, 0]
    for temp in (0.3, 0.7, 2.0):
        case = build_case("trained", dtype, vocab, vocab, temperature=temp)
        run_variants(libprl, cuda_device, monkeypatch, case, dtype, vocab, "trained", variants)
    case = build_case("offset_1000", dtype, vocab, vocab, temperature=1.0)
    run_variants(libprl, cuda_device, monkeypatch, case, dtype, vocab, "offset_1000", variants)
