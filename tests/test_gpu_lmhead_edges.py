"""The fused head's backward (csrc/prl_lmhead_bwd.hip through `FusedLmHead.backward_from_token_grads`) checked ENTRY BY ENTRY
(tests/head_grad_checks.py) with inputs placed where a wrong index shows: label, a maximum (+10) and exactly tied maxima on
the first / last vocabulary row of the tiles of all three workgroup shapes, of the partly masked last tile, and on both sides
of every split-K / vocabulary-range boundary; live token rows on the first / last row of a token tile and on both sides of every
chunk boundary; rows without a gradient in the middle of a tile; [B, L] layouts whose last row per sequence must stay exactly
zero; and weights / hidden states as a trained model makes them.  The token gradients are CHOSEN (no loss kernel in the loop),
`lse2` and the entropy come from the head's own forward, which is held to fp64 as well.

`build_head_case` runs on the CPU: tests/test_head_grad_checks_host.py measures the reference's fp32 arithmetic on the same
inputs, which is where every bound comes from."""

import math

import numpy as np
import pytest
import torch

import grad_checks as gc
import head_grad_checks as hg

pytestmark = pytest.mark.gpu

TILES = ["256x256", "256", "128", None]
TILE_IDS = ["tile256x256", "tile256x128_ring3", "tile128x128", "default_dispatch"]


def all_edges(V, T, chunk_rows=None, ksplit=(), nsplit=()):
    """Union of `edge_positions` over the three workgroup shapes."""
    vocab, token = set(), set()
    for bm, bn in hg.TILE_SHAPES.values():
        e = hg.edge_positions(V, T, bm, bn, chunk_rows, ksplit, nsplit)
        vocab |= set(e["vocab"])
        token |= set(e["token"])
    return sorted(vocab), sorted(token)


def build_head_case(family, B, L, H, V, weight_dtype=torch.float32, temperature=0.7, seed=0, chunk_rows=None, ksplit=(), nsplit=(),
                    entropy_grad=True):
    """CPU tensors of one problem: hidden [B, L, H] bf16, weight [V, H], input_ids [B, L], token-aligned g_nlp / g_ent [B, L]
    (element u belongs to logits row u - 1; column 0 is never read and holds 7.0), and the per-row (row_ids, g, gh)."""
    T = B * L
    gen = torch.Generator(device="cpu").manual_seed(seed)
    hidden = torch.randn(T, H, generator=gen) * (8.0 if family == "hidden_x8" else 1.0)
    W = torch.randn(V, H, generator=gen) * (2.0 / H ** 0.5)
    rng = np.random.default_rng(seed + 1)
    ids = rng.integers(0, V, size=T, dtype=np.int64)       # ids[q + 1] is the label of logits row q
    g = rng.normal(0.0, 1.0, T)
    gh = 0.05 * rng.normal(0.0, 1.0, T) if entropy_grad else np.zeros(T)
    gh[rng.random(T) < 0.25] = 0.0                          # rows without an entropy gradient take another branch
    if family in ("edges", "randn"):
        g[rng.random(T) < 0.05] = 0.0                       # an entropy gradient alone
    else:
        # p(label) ~ 1: ln p + H cancels to nothing and fp32 (the reference's z - logsumexp as much as a kernel's) has no digits
        # of it left; the reference loss never sends an entropy gradient without a policy gradient of ordinary size
        g = np.sign(g) * (0.2 + np.abs(g))
    dead = rng.random(T) < 0.1
    dead[41:46] = True                                      # a run of rows without any gradient inside a tile
    can_live = (np.arange(T) % L) != L - 1                  # logits row q predicts token q + 1 of the same sequence
    hidden = hidden.to(torch.bfloat16)
    unit = hidden.float() / hidden.float().pow(2).sum(-1, keepdim=True).clamp_min(1e-6)  # W[v] += a unit[q]: logit (q, v) += a

    if family == "edges":
        vocab_edges, token_edges = all_edges(V, T, chunk_rows, ksplit, nsplit)
        first = [q for q in token_edges if can_live[q]] + [q - 1 for q in token_edges if not can_live[q] and q >= 1 and can_live[q - 1]]
        rest = [int(q) for q in rng.permutation(T) if can_live[q] and q not in first]
        pool = first + rest
        for j, e in enumerate(vocab_edges):
            r1, r2, r3 = (pool[(3 * j + i) % len(pool)] for i in range(3))
            dead[[r1, r2, r3]] = False
            g[r1] = g[r1] or 0.5
            g[r3] = g[r3] or -0.5
            ids[r1 + 1] = e                                 # the label on the edge, an ordinary probability
            W[e] += 10.0 * unit[r2]                         # the row's maximum on the edge, its label elsewhere
            W[e] += 10.0 * unit[r3]                         # label and maximum on the edge
            ids[r3 + 1] = e
        for a, b in zip(vocab_edges[0::2], vocab_edges[1::2]):
            W[b] = W[a]                                     # equal weight rows: logits tied exactly, the maxima above included
    elif family == "trained":
        live = np.flatnonzero(can_live & ~dead)
        boost = rng.uniform(0.0, 25.0, T) * temperature     # p(label) from ~1 / V to ~1
        for q in live:
            W[ids[q + 1]] += float(boost[q]) * unit[q]
        if weight_dtype == torch.bfloat16:
            # a common logit offset (every weight row moved by the same vector: row q's logits move by hidden[q] . c, +-30).
            # Only where the weight is its own exact plane: through an fp32 weight the two bf16 planes carry the offset to
            # 2^-16 of ITS size in every logit, a cost of the documented operand format and no arithmetic error.
            W += torch.randn(H, generator=gen) * (30.0 / H ** 0.5)
        W[V // 2: V // 2 + min(1000, V // 4)] = 0.0          # zero weight rows: a flat stretch of every logits row
        hidden[7] = 0.0                                     # and one logits row that is flat altogether (p = 1 / V)
        dead[7] = False
        g[7] = g[7] or 0.3
    elif family not in ("randn", "hidden_x8"):
        raise ValueError(family)

    W = W.to(weight_dtype)
    g[dead | ~can_live] = 0.0
    gh[dead | ~can_live] = 0.0
    tok = lambda a: np.concatenate([[7.0], a[:-1]]).astype(np.float32).reshape(B, L)  # noqa: E731 - row q -> token q + 1
    g_tok, gh_tok = tok(g), tok(gh)
    g_tok[:, 0] = 7.0  # the first token of a sequence has no prediction: never read
    gh_tok[:, 0] = 7.0
    input_ids = ids.reshape(B, L)
    rid, g_row, gh_row = gc.token_rows(input_ids, g_tok[:, 1:], gh_tok[:, 1:])
    return {"family": family, "B": B, "L": L, "H": H, "V": V, "temperature": temperature, "hidden": hidden.reshape(B, L, H), "weight": W,
            "input_ids": torch.from_numpy(input_ids), "g_nlp": torch.from_numpy(g_tok), "g_ent": torch.from_numpy(gh_tok) if entropy_grad else None,
            "row_ids": rid, "g": g_row, "gh": gh_row, "can_live": can_live}


def _set_env(monkeypatch, **env):
    for k, v in env.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))


def run_and_check(case, dev, *, keep, chunk_rows=None, tile=None, terms=3, upstream=None, dh_dtypes=(torch.float32, torch.bfloat16),
                  dw_modes=("overwrite", "accumulate"), witness=None, label=""):
    """Forward + backward of one case on the device; asserts the forward bound and the per-entry bounds of d hidden and d W.
    Returns the witness terms (shared by the variants of a case) and the measured (d hidden, d W) errors."""
    from pipelinerl_amd.fused_head import FusedLmHead

    B, L, H, V, temp, fam = case["B"], case["L"], case["H"], case["V"], case["temperature"], case["family"]
    hidden, W, ids = case["hidden"].to(dev), case["weight"].to(dev), case["input_ids"].to(dev)
    g_nlp = case["g_nlp"].to(dev)
    g_ent = case["g_ent"].to(dev) if case["g_ent"] is not None else None
    up = torch.tensor(upstream, dtype=torch.float32, device=dev) if upstream is not None else None
    scale = 1.0 if upstream is None else float(up)
    head = FusedLmHead(W, hidden_grad_terms=terms, **({"chunk_rows": chunk_rows} if chunk_rows else {}))
    out = head.logprob_entropy(hidden, ids, temp, keep=keep)
    nlp, ent, lse2, h = out[:4]
    kept = out[4] if keep else None
    h2 = hidden.reshape(B * L, H)
    if witness is None:
        witness = hg.dlogits_terms(h2, W, case["row_ids"], case["g"] * scale, case["gh"] * scale, temp)
    # the forward outputs the backward consumes, against fp64 (token u = row u - 1; the first token of a sequence is 0)
    w_nlp, w_ent, w_lse = gc.forward_witness(witness[3], case["row_ids"], temp, row_block=64)
    pred = case["can_live"]
    tok = np.flatnonzero(pred) + 1
    fwd = 0.0
    for got, want in ((nlp, w_nlp), (ent, w_ent), (lse2 * math.log(2.0), w_lse)):
        got = got.double().cpu().numpy().reshape(-1)
        assert not got.reshape(B, L)[:, 0].any()
        fwd = max(fwd, float(np.abs(got[tok] - want[pred]).max()))
    print(f"{label} forward: {fwd:.3e} nats (bound {hg.HEAD_FWD_BOUND[fam]:.2e})")
    assert fwd <= hg.HEAD_FWD_BOUND[fam], (label, fwd)

    bm, bn = hg.TILE_SHAPES.get(tile, (None, None))
    worst = [0.0, 0.0]
    for dt in dh_dtypes:
        for mode in dw_modes:
            if mode == "overwrite":
                base, gw = None, torch.full((V, H), float("nan"), device=dev)
            else:
                base = torch.randn(V, H, generator=torch.Generator(device="cpu").manual_seed(5))
                base[1::2] *= 1e-3  # every other vocabulary row small: 2^-24 |base| stays below the bound of small d W entries there
                base = base.to(dev)
                gw = base.clone()
            # the backward's workspace (d logits planes, split-K partials) may be uninitialised: fill it with NaN patterns, so that a
            # store the kernels skip cannot be covered by what an earlier run of the same shape left in the reused allocation
            head._workspace("bwd", B, L, dev, chunk_rows or head.chunk_rows).fill_(0xFF)
            gh = head.backward_from_token_grads(h, ids, temp, lse2, ent, g_nlp, g_ent, up, grad_weight=gw, grad_hidden_dtype=dt,
                                                overwrite_weight_grad=mode == "overwrite", kept_logits=kept)
            torch.cuda.synchronize()
            assert gh.dtype == dt
            res_h, res_w = hg.head_errors(gh.reshape(B * L, H), gw, h2, W, None, None, None, temp, terms=witness,
                                          dh_rounding=gc.BF16_ROUNDING if dt == torch.bfloat16 else 0.0, dw_base=base, bm=bm, bn=bn,
                                          chunk_rows=chunk_rows or head.chunk_rows)
            b_h, b_w = hg.head_bound(fam, "d_hidden", W.dtype, terms), hg.head_bound(fam, "d_weight", W.dtype)
            print(f"{label} {str(dt)[6:]} {mode}: d hidden {res_h.err:.3e} (bound {b_h:.2e}), d W {res_w.err:.3e} (bound {b_w:.2e})")
            assert res_h.ok(b_h), f"{label} {dt} {mode}: {res_h}"
            assert res_w.ok(b_w), f"{label} {dt} {mode}: {res_w}"
            # rows that predict nothing: exactly zero, sequence ends included
            assert not gh.reshape(B * L, H)[torch.from_numpy(~pred).to(dev)].any()
            if dt == torch.float32:
                worst = [max(worst[0], res_h.err), max(worst[1], res_w.err)]
    return witness, worst


MID = (900, 512, 8256)  # many tiles in every direction; the last vocabulary tile is partial for every shape (8256 = 32 x 256 + 64)


@pytest.mark.parametrize("tile", TILES, ids=TILE_IDS)
def test_edge_placement_mid_shape(libprl, cuda_device, monkeypatch, tile):
    """Label / maximum / tied maxima on every tile edge of all three shapes, live rows on the token-tile edges: kept and
    recomputed logits, fp32 and bf16 d hidden, d W overwritten (over NaN) and accumulated."""
    _set_env(monkeypatch, PRL_LMHEAD_TILE=tile, PRL_LMHEAD_KSPLIT=None, PRL_LMHEAD_NSPLIT=None)
    T, H, V = MID
    case = build_head_case("edges", 1, T, H, V, seed=11)
    w = None
    for keep in (True, False):
        w, _ = run_and_check(case, cuda_device, keep=keep, tile=tile, witness=w, label=f"mid {tile} keep={keep}")


@pytest.mark.parametrize("tile", ["256x256", None], ids=["tile256x256", "default_dispatch"])
def test_edge_placement_mid_shape_bf16_weight(libprl, cuda_device, monkeypatch, tile):
    """The same placement with a bf16 weight (one exact plane: the generic 64-deep forward stream, the two-product d hidden)."""
    _set_env(monkeypatch, PRL_LMHEAD_TILE=tile, PRL_LMHEAD_KSPLIT=None, PRL_LMHEAD_NSPLIT=None)
    T, H, V = MID
    case = build_head_case("edges", 1, T, H, V, weight_dtype=torch.bfloat16, seed=11)
    w = None
    for keep in (True, False):
        w, _ = run_and_check(case, cuda_device, keep=keep, tile=tile, witness=w, label=f"mid bf16 weight {tile} keep={keep}")


@pytest.mark.parametrize("tile", ["256x256", "256", "128"], ids=TILE_IDS[:3])
@pytest.mark.parametrize("chunk", [100, 299])
def test_chunk_boundaries_per_tile_shape(libprl, cuda_device, monkeypatch, chunk, tile):
    """Chunk boundaries under each forced workgroup shape of the recompute (the kept-logits pass has no tile shape)."""
    _set_env(monkeypatch, PRL_LMHEAD_TILE=tile, PRL_LMHEAD_KSPLIT=None, PRL_LMHEAD_NSPLIT=None)
    case = build_head_case("edges", 2, 330, 128, 1088, seed=23, chunk_rows=chunk)
    run_and_check(case, cuda_device, keep=False, chunk_rows=chunk, tile=tile, label=f"chunk {chunk} {tile} recompute")


@pytest.mark.parametrize("wdt", [torch.float32, torch.bfloat16], ids=["f32_weight", "bf16_weight"])
@pytest.mark.parametrize("chunk", [100, 128, 299, None])
def test_chunk_boundaries(libprl, cuda_device, monkeypatch, chunk, wdt):
    """Live rows and edge labels on both sides of every chunk boundary, chunks that neither divide the rows nor are
    multiples of 128, over two sequences."""
    _set_env(monkeypatch, PRL_LMHEAD_TILE=None, PRL_LMHEAD_KSPLIT=None, PRL_LMHEAD_NSPLIT=None)
    case = build_head_case("edges", 2, 330, 128, 1088, weight_dtype=wdt, seed=23, chunk_rows=chunk)
    w = None
    for keep in (True, False):
        w, _ = run_and_check(case, cuda_device, keep=keep, chunk_rows=chunk, witness=w, label=f"chunk {chunk} keep={keep}")


@pytest.mark.parametrize("tile", ["256x256", "256", "128"], ids=TILE_IDS[:3])
@pytest.mark.parametrize("env,value", [("PRL_LMHEAD_KSPLIT", 2), ("PRL_LMHEAD_KSPLIT", 3), ("PRL_LMHEAD_KSPLIT", 8),
                                       ("PRL_LMHEAD_NSPLIT", 1), ("PRL_LMHEAD_NSPLIT", 3), ("PRL_LMHEAD_NSPLIT", 64)])
def test_vocabulary_slice_boundaries(libprl, cuda_device, monkeypatch, tile, env, value):
    """Labels and maxima on both sides of every split-K slice of d hidden's contraction and of every vocabulary range of the
    d logits recompute."""
    _set_env(monkeypatch, PRL_LMHEAD_TILE=tile, PRL_LMHEAD_KSPLIT=None, PRL_LMHEAD_NSPLIT=None)
    monkeypatch.setenv(env, str(value))
    ks = (value,) if env.endswith("KSPLIT") else ()
    ns = (value,) if env.endswith("NSPLIT") else ()
    case = build_head_case("edges", 1, 300, 128, 4160, seed=33, ksplit=ks, nsplit=ns)
    run_and_check(case, cuda_device, keep=False, tile=tile, dw_modes=("overwrite",), label=f"{env}={value} {tile} recompute")
    if ks:
        run_and_check(case, cuda_device, keep=True, tile=tile, dw_modes=("overwrite",), label=f"{env}={value} {tile} kept")


@pytest.mark.parametrize("B", [1, 2, 3])
def test_batch_layouts_no_entropy_gradient_and_upstream(libprl, cuda_device, monkeypatch, B):
    """[B, L]: the last row of every sequence is exactly zero in d hidden and adds nothing to d W; `g_ent = None`; an
    upstream scalar scales both."""
    _set_env(monkeypatch, PRL_LMHEAD_TILE=None, PRL_LMHEAD_KSPLIT=None, PRL_LMHEAD_NSPLIT=None)
    L = 390 // B
    for ent_grad, up in ((True, None), (False, None), (True, 0.25)):
        case = build_head_case("edges", B, L, 128, 1088, seed=40 + B, entropy_grad=ent_grad)
        for keep in (True, False):
            run_and_check(case, cuda_device, keep=keep, upstream=up, dw_modes=("overwrite",),
                          label=f"B={B} gH={'yes' if ent_grad else 'None'} upstream={up} keep={keep}")


FAMILY_CASES = [(f, t, w) for w in (torch.float32, torch.bfloat16) for f, t in (("randn", 0.7), ("trained", 0.3), ("trained", 0.7), ("trained", 2.0))]
FAMILY_CASES.append(("hidden_x8", 0.7, torch.bfloat16))


@pytest.mark.parametrize("family,temp,wdt", FAMILY_CASES, ids=[f"{f}-T{t}-{str(w)[6:]}" for f, t, w in FAMILY_CASES])
def test_input_families(libprl, cuda_device, monkeypatch, family, temp, wdt):
    """Weights aligned with the hidden states (p(label) up to ~1), a flat row, flat stretches, a common offset (bf16 weight),
    three temperatures; hidden states of eight times the size with a bf16 weight (an fp32 weight's two planes give every logit
    to 2^-16 of sum |h| |W|, eight times more here: the documented format alone moves the probabilities by 1e-4)."""
    _set_env(monkeypatch, PRL_LMHEAD_TILE=None, PRL_LMHEAD_KSPLIT=None, PRL_LMHEAD_NSPLIT=None)
    case = build_head_case(family, 1, 300, 256, 4160, weight_dtype=wdt, temperature=temp, seed=51)
    w = None
    for keep in (True, False):
        w, _ = run_and_check(case, cuda_device, keep=keep, witness=w, dw_modes=("overwrite",), label=f"{family} T={temp} keep={keep}")


@pytest.mark.parametrize("tile", ["256x256", "256", "128"], ids=TILE_IDS[:3])
@pytest.mark.parametrize("T,H,V", [(130, 64, 192), (257, 128, 320), (64, 192, 4160), (300, 64, 1088), (900, 128, 1088)])
def test_small_ragged_shapes_per_entry(libprl, cuda_device, monkeypatch, tile, T, H, V):
    """The ragged shapes of test_gpu_lmhead_fused.test_small_ragged_shapes with placed edges, per entry."""
    _set_env(monkeypatch, PRL_LMHEAD_TILE=tile, PRL_LMHEAD_KSPLIT=None, PRL_LMHEAD_NSPLIT=None)
    case = build_head_case("edges", 1, T, H, V, seed=T)
    w = None
    for keep in (True, False):
        w, _ = run_and_check(case, cuda_device, keep=keep, tile=tile, witness=w, dw_modes=("overwrite",), label=f"{T}x{H}x{V} {tile} keep={keep}")


@pytest.mark.parametrize("H,V,wdt", [(3584, 152064, torch.float32), (896, 151936, torch.bfloat16)], ids=["qwen7b_f32", "qwen0p5b_bf16"])
def test_baseline_head_shapes_per_entry(libprl, cuda_device, monkeypatch, H, V, wdt):
    """The two BASELINE head shapes, 160 rows, default dispatch, kept and recomputed."""
    _set_env(monkeypatch, PRL_LMHEAD_TILE=None, PRL_LMHEAD_KSPLIT=None, PRL_LMHEAD_NSPLIT=None)
    case = build_head_case("edges", 1, 160, H, V, weight_dtype=wdt, seed=3)
    w = None
    for keep in (True, False):
        w, _ = run_and_check(case, cuda_device, keep=keep, witness=w, dw_modes=("overwrite",), label=f"H={H} V={V} keep={keep}")


@pytest.mark.parametrize("terms", [1, 2])
def test_reduced_hidden_gradient_terms_have_their_own_allowance(libprl, cuda_device, monkeypatch, terms):
    """`hidden_grad_terms` 1 / 2 drop operand planes: inside their derived allowance (2^-8 per dropped plane), and OUTSIDE
    the default path's bound - the default cannot silently become one of them.  d W is unaffected."""
    _set_env(monkeypatch, PRL_LMHEAD_TILE=None, PRL_LMHEAD_KSPLIT=None, PRL_LMHEAD_NSPLIT=None)
    case = build_head_case("randn", 1, 200, 256, 2048, seed=13)
    _, (e_h, _) = run_and_check(case, cuda_device, keep=False, terms=terms, dh_dtypes=(torch.float32,), dw_modes=("overwrite",),
                                label=f"hidden_grad_terms={terms}")
    assert e_h > hg.head_bound("randn", "d_hidden", torch.float32, 3), e_h
