"""The per-entry check of the fused head's d hidden / d W (tests/head_grad_checks.py) tested on the CPU: what it accepts
(the reference's fp32 arithmetic, the documented operand format emulated without the package), what it rejects (d logits
wrong on purpose, carried through the two products in fp64), and that the max-norm assertions the head's tests used alone
until now accept most of what it rejects.  Nothing here runs a kernel; the inputs are the GPU suite's own
(`test_gpu_lmhead_edges.build_head_case`, and the `_problem` recipe of test_gpu_lmhead_fused.py)."""

import numpy as np
import pytest
import torch

import grad_checks as gc
import head_grad_checks as hg
import test_gpu_lmhead_edges as edges
from helpers import rel_err

F32_TOL, BF16_TOL = 1e-4, 4e-3  # what test_gpu_lmhead_fused.py allows under rel_err (fp32 / bf16-delivered gradients)


def _suite_problem(T, H, V, seed=0, temperature=0.7):
    """The input recipe of test_gpu_lmhead_fused._problem with chosen token gradients: W = randn * 2 / sqrt(H), bf16 randn
    hidden, random labels, ~20 % rows without a label, g ~ N(0, 1) / T, gH = -0.01 / T."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    hidden = torch.randn(T, H, generator=gen).to(torch.bfloat16)
    W = torch.randn(V, H, generator=gen) * (2.0 / H ** 0.5)
    rng = np.random.default_rng(seed + 1)
    ids = rng.integers(0, V, size=T)
    live = rng.random(T) >= 0.2
    live[-1] = False
    live[0] = True
    g = np.where(live, rng.normal(0, 1, T) / temperature, 0.0)
    gh = np.where(live, -0.01 / temperature, 0.0)
    return hidden, W, ids, g, gh, temperature


def _mutants(want, scale, x, ids, g, gh, temp):
    """name -> d logits [R, V] fp64 wrong on purpose (torch)."""
    R, V = want.shape
    live = np.flatnonzero(g != 0)
    is_label = torch.zeros((R, V), dtype=torch.bool)
    is_label[torch.from_numpy(live), torch.from_numpy(ids[live])] = True
    out = {}
    hi = want.float().to(torch.bfloat16).double()
    out["d-logits low plane dropped"] = hi
    no_ent, _, _ = zip(*[gc._witness_block(x[a:a + 32], torch.from_numpy(ids[a:a + 32]), torch.from_numpy(g[a:a + 32]),
                                           torch.zeros(len(g[a:a + 32]), dtype=torch.float64), temp) for a in range(0, R, 32)])
    out["entropy term dropped"] = torch.cat(no_ent)
    m = want.clone()
    m[:, V - 8:] = torch.where(is_label[:, V - 8:], m[:, V - 8:], torch.zeros(()).double())
    out["last 8 vocabulary columns zero"] = m
    c = next(c for c in range(V // 2, V) if not is_label[:, c].any() and not is_label[:, c + 1].any())
    m = want.clone()
    m[:, c] = m[:, c + 1]
    out["one column holds its neighbour's values"] = m
    for f in (1.001, 1.0003):
        out[f"softmax body x {f}"] = torch.where(is_label, want, want * f)
    m = want.clone()
    small = live[np.argsort(np.abs(g[live]))[:7]]
    m[torch.from_numpy(small)] *= 1.005
    out["the 7 live rows with the smallest |g| x 1.005"] = m
    return out


# what the max norm is expected to accept (the documented gap).  bf16 at 4e-3: everything but the dropped entropy term;
# fp32 at 1e-4: a body off by 3e-4 (the rows with the smallest |g| x 1.005 score 1.2e-4 / 1.1e-4 on these inputs, 5.7e-5 /
# 4.1e-5 on the issue's: at the edge of that tolerance either way, so only the bf16 tolerance is asserted for them)
OLD_F32_ACCEPTS = ("softmax body x 1.0003",)


@pytest.mark.parametrize("T,H,V", [(257, 128, 320), (160, 256, 152064)], ids=["small", "full_vocab"])
def test_mutants_are_rejected_and_the_max_norm_accepts_them(T, H, V):
    hidden, W, ids, g, gh, temp = _suite_problem(T, H, V, seed=T)
    terms = hg.dlogits_terms(hidden, W, ids, g, gh, temp)
    want, scale, _, x = terms
    dh64, dw64 = hg.products64(want, hidden, W)
    b_h, b_w = hg.head_bound("randn", "d_hidden"), hg.head_bound("randn", "d_weight")

    # honest candidates: the reference's fp32 arithmetic and the documented operand format
    ref = gc.reference_fp32(None, ids, g, gh, temp, hidden=hidden, weight=W, row_block=64)
    emu = hg.emulate_planes(want, hidden, W)
    for name, (dh, dw) in (("reference fp32", (ref[4], ref[5])), ("operand format emulated", emu)):
        for bf16 in (False, True):
            a = gc.round_bf16(np.asarray(dh, dtype=np.float32)) if bf16 else dh
            b = gc.round_bf16(np.asarray(dw, dtype=np.float32)) if bf16 else dw
            r = gc.BF16_ROUNDING if bf16 else 0.0
            res_h, res_w = hg.head_errors(a, b, hidden, W, None, None, None, temp, terms=terms, dh_rounding=r, dw_rounding=r)
            print(f"{name} bf16={bf16}: d hidden {res_h.err:.3e} (bound {b_h:.2e}), d W {res_w.err:.3e} (bound {b_w:.2e})")
            assert res_h.ok(b_h) and res_w.ok(b_w), f"{name}: {res_h}; {res_w}"

    for name, dl in _mutants(want, scale, x, ids, g, gh, temp).items():
        dh, dw = hg.products64(dl, hidden, W)
        for bf16 in (False, True):
            a = gc.round_bf16(dh.numpy()) if bf16 else dh
            b = gc.round_bf16(dw.numpy()) if bf16 else dw
            r = gc.BF16_ROUNDING if bf16 else 0.0
            res_h, res_w = hg.head_errors(a, b, hidden, W, None, None, None, temp, terms=terms, dh_rounding=r, dw_rounding=r)
            old_h, old_w = rel_err(np.asarray(a, dtype=np.float64), dh64.numpy()), rel_err(np.asarray(b, dtype=np.float64), dw64.numpy())
            print(f"mutant '{name}' bf16={bf16}: per-entry d hidden {res_h.err:.2e} d W {res_w.err:.2e}; max norm {old_h:.2e} / {old_w:.2e}")
            assert not res_h.ok(b_h), f"'{name}' must be rejected in d hidden: {res_h}"
            assert not res_w.ok(b_w), f"'{name}' must be rejected in d W: {res_w}"
            if V == 152064:  # the gap, as measured for the issue at this shape
                if bf16 and name != "entropy term dropped":  # 6e-3 / 7.5e-3 here: the one mutant the bf16 tolerance does see
                    assert old_h <= BF16_TOL and old_w <= BF16_TOL, (name, old_h, old_w)
                elif name in OLD_F32_ACCEPTS:
                    assert old_h <= F32_TOL and old_w <= F32_TOL, (name, old_h, old_w)


def test_weight_low_plane_dropped_and_the_reduced_terms_allowance():
    """`hidden_grad_terms` = 2 / 1 emulated: outside the default bound (the default cannot silently become one of them), inside
    their own derived allowance; the max norm at the bf16 tolerance accepts both."""
    case = edges.build_head_case("randn", 1, 200, 256, 2048, seed=13)
    hidden, W, temp = case["hidden"][0], case["weight"], case["temperature"]
    terms = hg.dlogits_terms(hidden, W, case["row_ids"], case["g"], case["gh"], temp)
    dh64, _ = hg.products64(terms[0], hidden, W)
    for t in (2, 1):
        dh, _ = hg.emulate_planes(terms[0], hidden, W, t)
        res, _ = hg.head_errors(dh, None, hidden, W, None, None, None, temp, terms=terms)
        print(f"hidden_grad_terms={t}: per-entry {res.err:.3e}, allowance {hg.head_bound('randn', 'd_hidden', terms=t):.3e}, max norm {rel_err(dh.numpy(), dh64.numpy()):.2e}")
        assert not res.ok(hg.head_bound("randn", "d_hidden"))
        assert res.ok(hg.head_bound("randn", "d_hidden", terms=t)), str(res)
        assert rel_err(dh.numpy(), dh64.numpy()) <= BF16_TOL


REF_CASES = [
    ("edges", dict(B=1, L=900, H=512, V=8256, seed=11)),
    ("edges", dict(B=1, L=900, H=512, V=8256, seed=11, weight_dtype=torch.bfloat16)),
    ("edges", dict(B=2, L=330, H=128, V=1088, seed=23, chunk_rows=100)),
    ("edges", dict(B=2, L=330, H=128, V=1088, seed=23, chunk_rows=299, weight_dtype=torch.bfloat16)),
    ("edges", dict(B=1, L=300, H=128, V=4160, seed=33, ksplit=(3,))),
    ("edges", dict(B=1, L=300, H=128, V=4160, seed=33, nsplit=(64,))),
    ("edges", dict(B=3, L=130, H=128, V=1088, seed=43, entropy_grad=False)),
    ("edges", dict(B=1, L=64, H=192, V=4160, seed=64)),
    ("edges", dict(B=1, L=160, H=896, V=151936, seed=3, weight_dtype=torch.bfloat16)),
    ("randn", dict(B=1, L=300, H=256, V=4160, seed=51)),
    ("randn", dict(B=1, L=200, H=256, V=2048, seed=13)),
    ("trained", dict(B=1, L=300, H=256, V=4160, seed=51, temperature=0.3)),
    ("trained", dict(B=1, L=300, H=256, V=4160, seed=51, temperature=0.7, weight_dtype=torch.bfloat16)),
    ("trained", dict(B=1, L=300, H=256, V=4160, seed=51, temperature=2.0)),
    ("hidden_x8", dict(B=1, L=300, H=256, V=4160, seed=51, weight_dtype=torch.bfloat16)),
]


@pytest.mark.parametrize("family,kw", REF_CASES, ids=[f"{f}-{i}" for i, (f, _) in enumerate(REF_CASES)])
def test_reference_and_format_stay_within_the_written_values(family, kw):
    """Re-measures on the GPU cases' own inputs: the reference's fp32 arithmetic <= HEAD_REF / HEAD_FWD_REF, the emulated
    operand format <= HEAD_FORMAT, every default bound below the mutant floor."""
    case = edges.build_head_case(family, **kw)
    hidden, W, temp = case["hidden"].reshape(-1, case["H"]), case["weight"], case["temperature"]
    terms = hg.dlogits_terms(hidden, W, case["row_ids"], case["g"], case["gh"], temp)
    ref = gc.reference_fp32(None, case["row_ids"], case["g"], case["gh"], temp, hidden=hidden, weight=W, row_block=64)
    res_h, res_w = hg.head_errors(ref[4], ref[5], hidden, W, None, None, None, temp, terms=terms)
    pred = case["can_live"]
    fwd = max(float(np.abs(a[pred].astype(np.float64) - b[pred]).max()) for a, b in zip(ref[1:4], gc.forward_witness(terms[3], case["row_ids"], temp, row_block=64)))
    emu_h, emu_w = hg.head_errors(*hg.emulate_planes(terms[0], hidden, W), hidden, W, None, None, None, temp, terms=terms)
    print(f"{family} {kw}: reference d hidden {res_h.err:.3e} d W {res_w.err:.3e} forward {fwd:.3e}; format d hidden {emu_h.err:.3e} d W {emu_w.err:.3e}")
    assert res_h.stray == 0 and res_h.err <= hg.HEAD_REF[family]["d_hidden"], str(res_h)
    assert res_w.stray == 0 and res_w.err <= hg.HEAD_REF[family]["d_weight"], str(res_w)
    assert fwd <= hg.HEAD_FWD_REF[family]
    assert emu_h.ok(hg.HEAD_FORMAT[hg.format_key("d_hidden", W.dtype)]), str(emu_h)
    assert emu_w.ok(hg.HEAD_FORMAT["d_weight"]), str(emu_w)
    for p in ("d_hidden", "d_weight"):
        assert hg.head_bound(family, p, W.dtype) < gc.MUTANT_FLOOR
    # rows that predict nothing are exactly zero in the witness' scale: a stray value there is counted
    dead = np.flatnonzero(~pred)
    bad = np.array(ref[4], copy=True)
    bad[dead[0], 3] = 1e-30
    assert hg.head_errors(bad, None, hidden, W, None, None, None, temp, terms=terms)[0].stray == 1


def test_accumulate_allows_one_rounding_of_the_buffer():
    case = edges.build_head_case("randn", 1, 64, 64, 192, seed=1)
    hidden, W, temp = case["hidden"][0], case["weight"], case["temperature"]
    terms = hg.dlogits_terms(hidden, W, case["row_ids"], case["g"], case["gh"], temp)
    _, dw = hg.products64(terms[0], hidden, W)
    base = torch.randn(192, 64, generator=torch.Generator().manual_seed(2)) * 100.0
    got = (base.double() + dw).float()  # one fp32 rounding of the sum
    assert hg.head_errors(None, got, hidden, W, None, None, None, temp, terms=terms, dw_base=base)[1].ok(1e-9)
    assert not hg.head_errors(None, got, hidden, W, None, None, None, temp, terms=terms)[1].ok(1e-3)  # the base is not part of d W
    got[5, 5] += 1e-3
    res = hg.head_errors(None, got, hidden, W, None, None, None, temp, terms=terms, dw_base=base, bm=128)[1]
    assert (res.row, res.col) == (5, 5) and not res.ok(1e-5) and "vocabulary tile 0 (row 5)" in res.where


def test_edge_positions_against_hand_worked_layouts():
    # V = 8256 = 32 x 256 + 64 = 64 x 128 + 64; 900 rows; chunks of 299
    e = hg.edge_positions(8256, 900, 256, 256, chunk_rows=299)
    assert e["vocab"] == [0, 255, 256, 8191, 8192, 8255]
    assert e["token"] == [0, 255, 256, 298, 299, 597, 598, 896, 897, 899]
    e = hg.edge_positions(8256, 900, 128, 128)
    assert e["vocab"] == [0, 127, 128, 8191, 8192, 8255] and e["token"] == [0, 127, 128, 899]
    # whole tiles only: no partial-tile entries, nothing outside the problem
    assert hg.edge_positions(1024, 100, 256, 128)["vocab"] == [0, 255, 256, 1023]
    assert hg.edge_positions(1024, 100, 256, 128)["token"] == [0, 99]
    # V = 4160 = 130 steps of 32: 2 slices of 65; 3 of 44 (44 + 44 + 42); 8 of 17 (7 x 17 + 11)
    assert hg.ksplit_boundaries(4160, 2) == [2080]
    assert hg.ksplit_boundaries(4160, 3) == [1408, 2816]
    assert hg.ksplit_boundaries(4160, 8) == [544 * i for i in range(1, 8)]
    assert hg.ksplit_boundaries(4160, 1) == [] and hg.ksplit_boundaries(128, 8) == []  # 4 steps: a request above steps / 2 is ignored
    # 4160 rows are 17 tiles of 256 (3 ranges: tiles 0-4, 5-10, 11-16) or 33 tiles of 128; more ranges than tiles: one each
    assert hg.nsplit_boundaries(4160, 256, 3) == [1280, 2816]
    assert hg.nsplit_boundaries(4160, 256, 64) == [256 * i for i in range(1, 17)]
    assert hg.nsplit_boundaries(4160, 128, 1) == []
    e = hg.edge_positions(4160, 300, 256, 128, ksplit=(2,), nsplit=(3,))
    assert e["vocab"] == [0, 255, 256, 1279, 1280, 2079, 2080, 2815, 2816, 4095, 4096, 4159]
    assert "chunk 1 row 1 of it, product tile (0, 1), d logits token tile 0 (row 1)" == hg.locate("d_hidden", 300, 300, bn=128, chunk_rows=299)
    assert hg.locate("d_weight", 8200, 10, bm=256) == "product tile (32, 0), d logits vocabulary tile 32 (row 8)"
    # every vocabulary edge of a built case carries a label, and its pair is tied exactly
    case = edges.build_head_case("edges", 1, 300, 128, 4160, seed=33, ksplit=(3,))
    ve, te = edges.all_edges(4160, 300, ksplit=(3,))
    live = case["g"] != 0
    assert set(ve) <= set(case["row_ids"][live].tolist())
    assert all(case["g"][q] != 0 or case["gh"][q] != 0 for q in te if q != 299)
    assert torch.equal(case["weight"][ve[0]], case["weight"][ve[1]])
    assert case["g"][299] == 0 and case["gh"][299] == 0 and case["row_ids"][299] == -1
