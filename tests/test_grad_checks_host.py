"""The per-entry d logits check (tests/grad_checks.py) tested on the CPU: what it accepts, what it rejects, and that
the max norm the suite used alone until now (`helpers.rel_err`) accepts every one of the rejected arrays.

Inputs are the GPU suite's own (`test_gpu_fullvocab._case`, `test_gpu_logits_edges.build_case`).  The mutants are numpy
edits of the oracle's gradient that imitate what a subtly wrong kernel writes: nothing here runs a kernel."""

import numpy as np
import pytest
import torch

import grad_checks as gc
import test_gpu_logits_edges as edges
from helpers import rel_err
from test_gpu_fullvocab import CONFIGS, FP_TOL, _case

BF16_TOL = 1e-2  # what the GPU tests allow a bf16 gradient under rel_err
FAMILY = "randn_spiky"
CASES = [(152064, 16, "kl_ent_temp"), (152064, 16, "grpo_clip"), (4099, 40, "kl_ent_temp")]


def _inputs(V, T, cfg_name, dtype):
    logits, batch, want, g64 = _case(V, T, cfg_name, dtype)
    rid, g, gh = gc.token_rows(batch["input_ids"], want["g_nlp"], want["g_ent"])
    return logits[0], rid, g, gh, CONFIGS[cfg_name]["temperature"], want["grad_logits"][0], g64


def _both(arr, dtype, x, rid, g, gh, temp, g64):
    """(per-entry result, rel_err against the fp64 witness, rel_err tolerance) of a candidate gradient."""
    if dtype == "bf16":
        arr = gc.round_bf16(arr)
    res = gc.dlogits_error(arr, x, rid, g, gh, temp, out_rounding=gc.BF16_ROUNDING if dtype == "bf16" else 0.0)
    return res, rel_err(arr, g64), (FP_TOL if dtype == "f32" else BF16_TOL)


def _mutants(V, x, rid, g, gh, temp, oracle, g64):
    """name -> mutated copy of the oracle's gradient."""
    T = oracle.shape[0]
    live = np.flatnonzero(g != 0)
    zero_rows = np.flatnonzero((g == 0) & (gh == 0))[:-1]
    is_label = np.zeros(oracle.shape, dtype=bool)
    is_label[live, rid[live]] = True
    small = np.abs(g64) < FP_TOL * np.abs(g64).max()  # what rel_err cannot see at all
    r = int(live[np.argmin(np.abs(g[live]))])         # a computed row, the one with the smallest token gradient
    out = {}

    m = oracle.copy()
    m[~is_label] *= np.float32(1.001)
    out["softmax body x 1.001"] = m

    m = oracle.copy()
    vmax = np.abs(g64[r, :V // 4 * 4]).reshape(-1, 4).max(-1)
    j = int(np.argmin(np.where(is_label[r, :V // 4 * 4].reshape(-1, 4).any(-1), np.inf, vmax)))
    m[r, 4 * j:4 * j + 4] = 0.0
    out["one 16-byte vector of one row not written"] = m

    if V % 4:
        m = oracle.copy()
        m[:, V // 4 * 4:][small[:, V // 4 * 4:]] = 0.0
        out["the last vocab % NV columns (scalar tail) not written"] = m

    # the vector tail of the kernel that takes this row by default (row-resident for V >= 102 400, else 1024 x 4)
    name = edges.expected_kernel(None, "f32", V, V + (-V) % 4)
    tail = [(lo, hi) for n, lo, hi in gc.regions_of_kernel(name, V) if n == "vector_tail"]
    if tail and tail[0][1] - tail[0][0] < V // 2:
        lo, hi = tail[0]
        m = oracle.copy()
        m[:, lo:hi][small[:, lo:hi]] = 0.0
        out["the vector tail not written"] = m

    m = oracle.copy()
    m[small] = 0.0
    out["every entry below 1e-4 x max set to zero"] = m

    # row r with lse2 off by 1e-3: p_v and ln p_v of the whole row shifted
    z = torch.from_numpy(x[r]).double() / temp
    logp = torch.log_softmax(z, -1)
    H = float(-(logp.exp() * logp).sum())
    logp = logp - 1e-3 * np.log(2.0)
    p = logp.exp()
    row = (-g[r]) * p - gh[r] * p * (logp + H)
    row[rid[r]] += g[r]
    m = oracle.copy()
    m[r] = (row / temp).numpy().astype(np.float32)
    out["one row computed with lse2 off by 1e-3"] = m

    m = oracle.copy()
    m[zero_rows[0], 77] = np.float32(1e-7 * np.abs(g64).max())
    out["a non-zero written into a row without gradient"] = m

    m = oracle.copy()
    m[T - 1, 5] = np.float32(1e-7 * np.abs(g64).max())
    out["a non-zero written into the last row"] = m
    return out


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("V,T,cfg_name", CASES)
def test_reference_and_oracle_pass_and_mutants_are_rejected(V, T, cfg_name, dtype):
    x, rid, g, gh, temp, oracle, g64 = _inputs(V, T, cfg_name, dtype)
    bound = gc.DLOGITS_BOUND[FAMILY]
    assert bound < gc.MUTANT_FLOOR

    # the reference's own fp32 arithmetic: the yardstick.  Its value may not exceed the one the bound was derived from.
    ref_grad = gc.reference_fp32(x, rid, g, gh, temp)[0]
    ref = gc.dlogits_error(ref_grad, x, rid, g, gh, temp)
    print(f"reference fp32 V={V} {cfg_name} {dtype}: {ref.err:.3e} (family value {gc.DLOGITS_REF[FAMILY]:.1e}, bound {bound:.1e})")
    assert ref.stray == 0 and ref.err <= gc.DLOGITS_REF[FAMILY], str(ref)
    for name, arr in (("reference fp32", ref_grad), ("oracle", oracle)):
        res, re_, tol = _both(arr, dtype, x, rid, g, gh, temp, g64)
        print(f"{name}: per-entry {res.err:.3e}, rel_err {re_:.3e}")
        assert res.ok(bound), f"{name}: {res}"
        assert re_ <= tol

    for name, arr in _mutants(V, x, rid, g, gh, temp, oracle, g64).items():
        res, re_, tol = _both(arr, dtype, x, rid, g, gh, temp, g64)
        print(f"mutant '{name}': per-entry {res.err:.3e} stray {res.stray}, rel_err {re_:.3e} (tolerance {tol:.0e})")
        assert not res.ok(bound), f"'{name}' must be rejected by the per-entry check: {res}"
        # the max norm does see a body scaled by 1.001 at its fp32 tolerance where a row has entries with p ~ 0.1 (the
        # spiky row: 1e-3 x 0.1 = 1e-4); at the bf16 tolerance it sees none of the mutants
        if dtype == "bf16" or name != "softmax body x 1.001":
            assert re_ <= tol, f"'{name}' is expected to pass the max-norm check (that is the gap): {re_}"


def test_worst_entry_is_located():
    """The message names row, column and kernel region of the worst entry."""
    x, rid, g, gh, temp, oracle, _ = _inputs(152064, 16, "kl_ent_temp", "f32")
    r = int(np.flatnonzero(g != 0)[3])
    c = 102400 + 8192 * 6 + 17  # inside the vector tail of the row-resident kernel at V = 152 064
    assert rid[r] != c
    m = oracle.copy()
    m[r, c] *= np.float32(1.5)
    regs = gc.regions_of_kernel("fused_logits_loss_keep_kernel<F32,1024,2,16,9,true>", 152064)
    assert [n for n, _, _ in regs] == ["register_head", "lds_head", "full_tiles", "vector_tail"]
    assert regs[0][1:] == (0, 16 * 1024 * 4) and regs[1][2] == 102400 and regs[2][2] == 102400 + 6 * 8192
    res = gc.dlogits_error(m, x, rid, g, gh, temp, regions=regs)
    assert (res.row, res.col) == (r, c) and res.region.startswith("vector_tail[151552,152064)"), str(res)
    assert "row %d col %d" % (r, c) in str(res)
    # regions of the other shapes
    assert gc.kernel_regions(4099, 4, 256, 4) == [("full_tiles", 0, 4096), ("scalar_tail", 4096, 4099)]
    assert gc.kernel_regions(4099, 4, 256, 4, vec_ok=False) == [("scalar_tail", 0, 4099)]
    assert gc.kernel_regions(102400, 4, 1024, 2, 16, 9) == [("register_head", 0, 65536), ("lds_head", 65536, 102400)]
    assert gc.kernel_regions(152067, 4, 1024, 2, 16, 9)[-1] == ("scalar_tail", 152064, 152067)


def test_nan_and_flushed_denormals():
    """A NaN anywhere is an error (in a live entry: infinite; in a zero entry: stray); an entry below the smallest
    normal fp32 number may be flushed to zero."""
    x = np.zeros((2, 8), dtype=np.float32)
    x[0, 1:] = -200.0  # p_v = e^-200: far below fp32, still > 0 in fp64
    ids, g, gh = np.array([0, 3]), np.array([1.0, 0.0]), np.array([0.0, 0.0])
    want, scale, _ = gc.dlogits_witness(x, ids, g, gh, 1.0)
    assert (scale[0] > 0).all() and not scale[1].any()
    got = want.astype(np.float32)
    assert not got[0, 1:].any()  # flushed
    assert gc.dlogits_error(got, x, ids, g, gh, 1.0).ok(1e-6)
    bad = got.copy()
    bad[0, 2] = np.nan
    assert not gc.dlogits_error(bad, x, ids, g, gh, 1.0).ok(1e-6)
    bad = got.copy()
    bad[1, 2] = np.nan
    assert gc.dlogits_error(bad, x, ids, g, gh, 1.0).stray == 1


@pytest.mark.parametrize("family,kind,dtype,vocab,stride,temp", [
    ("edges", "edges", "f32", 4099, 4104, 0.7), ("edges", "edges", "bf16", 16384, 16384, 0.7),
    ("trained", "trained", "f32", 152064, 152064, 0.3), ("trained", "trained", "bf16", 4099, 4099, 2.0),
    ("offset_1000", "offset_1000", "f32", 152064, 152064, 1.0), ("randn", "randn", "f32", 4100, 4100, 0.7),
])
def test_family_bounds_hold_for_the_reference(family, kind, dtype, vocab, stride, temp):
    """The reference's fp32 arithmetic on the GPU edge cases' own inputs stays within the value each family's bound was
    derived from (d logits per entry; log-prob / entropy / logsumexp absolute)."""
    case = edges.build_case(kind, dtype, vocab, stride, temperature=temp, rows=6 if kind == "randn" else 0)
    flat = case["logits"].reshape(-1, vocab)
    grad, nlp, ent, lse = gc.reference_fp32(flat, case["row_ids"], case["g"], case["gh"], temp)
    res = gc.dlogits_error(grad, flat, case["row_ids"], case["g"], case["gh"], temp)
    fwd = max(np.abs(got[:-1].astype(np.float64) - want[0, 1:]).max() for got, want in zip((nlp, ent, lse), case["fwd"]))
    print(f"{family} {dtype} V={vocab}: reference d logits {res.err:.3e} (<= {gc.DLOGITS_REF[family]:.1e}), forward {fwd:.3e} (<= {gc.FWD_REF[family]:.2e})")
    assert res.stray == 0 and res.err <= gc.DLOGITS_REF[family], str(res)
    assert fwd <= gc.FWD_REF[family]
    assert gc.DLOGITS_BOUND[family] < gc.MUTANT_FLOOR
