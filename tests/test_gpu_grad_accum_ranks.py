"""`grad_accumulate_ranks_kernel` (csrc/prl_optim.hip) through `prl_optim_grad_accumulate_ranks`: the `world` ranks' copies of every
piece, one stride apart in a receive buffer, folded into fp32 accumulators in one pass.

The result is an equality of bits with a numpy float32 emulation that adds in rank order - `(((acc + g_0) + g_1) + ...)`, or
`(((float)g_0 + g_1) + ...)` when overwriting (one IEEE add per term, a bf16 source widens exactly; any NaN equals any NaN).  The
inputs are N(0, 1) x a log-uniform scale over 12 decades, so that the sum depends on the order, with +-0, +-inf and NaN planted so that
every rank contributes each of them somewhere."""

import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CHUNK = 16384
NUMELS = [0, 1, 7, 15, 16, 17, CHUNK, CHUNK + 1, 3 * CHUNK + 5]
WORLDS = [1, 2, 3, 4, 5, 8]
GUARD = 16  # elements behind every accumulator that no fold may touch
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, -0.0], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def _cases():
    """(numel, bf16 source?, source off 16-byte alignment?, accumulator off alignment?): every numel in both dtypes three times over
    (more than one launch of 64 segments), the last round with views offset by one element."""
    cases = [(n, bf16, False, False) for _ in range(3) for n in NUMELS for bf16 in (True, False)]
    cases += [(n, bf16, s_off, a_off) for n in NUMELS[1:] for bf16 in (True, False) for s_off, a_off in ((True, False), (False, True), (True, True))][:30]
    assert len(cases) > 64
    return cases


def _draw(rng, n, world, bf16):
    """[world, n] float32 holding the values the device sees (bf16 sources: bf16-representable)."""
    g = (rng.normal(0.0, 1.0, (world, n)) * 10.0 ** rng.uniform(-6.0, 6.0, (world, n))).astype(np.float32)
    for r in range(world):
        k = min(n, len(SPECIALS))
        g[r, :k] = np.roll(SPECIALS, r)[:k]  # element j sees another special from every rank: inf - inf, 0 + -0, NaN + x, ...
    if bf16:
        g = torch.from_numpy(g).to(torch.bfloat16).float().numpy()
    return g


def _same(got, want):
    both_nan = np.isnan(got) & np.isnan(want)
    return both_nan | (got.view(np.uint32) == want.view(np.uint32))


@pytest.mark.parametrize("overwrite", [1, 0])
@pytest.mark.parametrize("world", WORLDS)
def test_fold_is_the_rank_ordered_fp32_sum_bit_for_bit(libprl, cuda_device, world, overwrite):
    from pipelinerl_amd import _lib

    rng = np.random.default_rng(100 * world + overwrite)
    cases = _cases()
    # the receive buffer: one slot per rank, every piece at the same offset in every slot
    at, offs = 0, []
    for n, bf16, s_off, _a in cases:
        isz = 2 if bf16 else 4
        offs.append(at + (isz if s_off else 0))
        at += -(-(n + 1) * isz // 16) * 16
    stride = at
    host = np.zeros((world, stride), dtype=np.uint8)
    grads, accs, want = [], [], []
    for (n, bf16, _s, a_off), off in zip(cases, offs):
        g = _draw(rng, n, world, bf16)
        grads.append(g)
        raw = (g.view(np.uint32) >> 16).astype(np.uint16) if bf16 else g
        if n:
            host[:, off:off + raw.dtype.itemsize * n] = np.ascontiguousarray(raw).view(np.uint8).reshape(world, -1)
        start = (rng.normal(0.0, 1.0, n) * 10.0 ** rng.uniform(-6.0, 6.0, n)).astype(np.float32)
        with np.errstate(all="ignore"):
            w = g[0].copy() if overwrite else start + g[0]
            for r in range(1, world):
                w = w + g[r]
        want.append(w)
        base = torch.full((n + 1 + GUARD,), 12345.0, dtype=torch.float32, device=cuda_device)
        acc = base[1:n + 1] if a_off else base[:n]
        acc.copy_(torch.full((n,), float("nan")) if overwrite else torch.from_numpy(start))  # overwriting: NaN shows that acc is not read
        assert n == 0 or (acc.data_ptr() % 16 != 0) == a_off
        accs.append((base, acc, a_off))
    recv = torch.from_numpy(host.reshape(-1)).to(cuda_device)
    assert recv.data_ptr() % 16 == 0 and stride % 16 == 0
    table = (_lib.PrlAccumRanksSegment * (len(cases) + 2))()
    for seg, (n, bf16, s_off, _a), off, (_b, acc, _o) in zip(table, cases, offs, accs):
        seg.src, seg.acc, seg.numel = recv.data_ptr() + off, acc.data_ptr(), n
        seg.src_dtype = _lib.PRL_DTYPE_BF16 if bf16 else _lib.PRL_DTYPE_F32
        assert ((recv.data_ptr() + off) % 16 != 0) == s_off
    table[len(cases)].numel, table[len(cases)].acc = 100, accs[-1][1].data_ptr()  # no source: skipped
    table[len(cases) + 1].src, table[len(cases) + 1].acc = recv.data_ptr(), accs[-1][1].data_ptr()  # numel 0: skipped
    _lib.check(libprl.prl_optim_grad_accumulate_ranks(table, len(table), world, stride, overwrite, _lib.current_stream_ptr(cuda_device)))
    torch.cuda.synchronize(cuda_device)
    for (n, bf16, s_off, a_off), (base, acc, _o), w, g in zip(cases, accs, want, grads):
        got = acc.cpu().numpy()
        same = _same(got, w)
        assert same.all(), (f"numel {n} bf16 {bf16} unaligned {s_off, a_off} world {world} overwrite {overwrite}: {int((~same).sum())} entries differ from "
                            f"the rank-ordered fp32 sum, first at {int(np.argmin(same))}")
        tail = base[n + 1:] if a_off else base[n:]
        assert torch.all(tail == 12345.0) and (not a_off or float(base[0]) == 12345.0), "the fold wrote outside its accumulator"
    # the inputs did exercise what they are for
    flat = np.concatenate([w for w in want if w.size >= 8])
    given = np.concatenate([g.ravel() for g in grads])
    assert (given == 0).any() and np.signbit(given[given == 0]).any() and np.isposinf(given).any() and np.isneginf(given).any() and np.isnan(given).any()
    assert not np.isfinite(flat).all(), "and they reach the results"
    if world >= 3:
        g = grads[max(range(len(cases)), key=lambda i: cases[i][0])]
        with np.errstate(all="ignore"):
            rev = functools.reduce(lambda a, b: a + b, list(g[::-1]))
            fwd = functools.reduce(lambda a, b: a + b, list(g))
        assert (rev[8:].view(np.uint32) != fwd[8:].view(np.uint32)).any(), "the sum of these inputs depends on the order"


def test_one_fused_fold_equals_world_separate_folds(libprl, cuda_device):
    """The promise the optimizer leans on: one call of the fused fold = `world` calls of `prl_optim_grad_accumulate`, in bits."""
    from pipelinerl_amd import _lib

    world, n = 5, 3 * CHUNK + 5
    rng = np.random.default_rng(5)
    g = torch.from_numpy(_draw(rng, n, world, True)).to(cuda_device, torch.bfloat16)
    stride = -(-n * 2 // 16) * 16
    recv = torch.zeros(world * stride, dtype=torch.uint8, device=cuda_device)
    recv.view(world, stride)[:, :2 * n] = g.view(torch.uint8).view(world, 2 * n)
    start = torch.from_numpy(rng.normal(0, 1, n).astype(np.float32)).to(cuda_device)
    fused, separate = start.clone(), start.clone()
    stream = _lib.current_stream_ptr(cuda_device)
    t = (_lib.PrlAccumRanksSegment * 1)()
    t[0].src, t[0].acc, t[0].numel, t[0].src_dtype = recv.data_ptr(), fused.data_ptr(), n, _lib.PRL_DTYPE_BF16
    _lib.check(libprl.prl_optim_grad_accumulate_ranks(t, 1, world, stride, 0, stream))
    for r in range(world):
        s = (_lib.PrlAccumSegment * 1)()
        s[0].grad, s[0].acc, s[0].numel, s[0].grad_dtype = g[r].data_ptr(), separate.data_ptr(), n, _lib.PRL_DTYPE_BF16
        _lib.check(libprl.prl_optim_grad_accumulate(s, 1, 0, stream))
    torch.cuda.synchronize(cuda_device)
    assert _same(fused.cpu().numpy(), separate.cpu().numpy()).all()
