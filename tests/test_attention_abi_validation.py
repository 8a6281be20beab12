"""The attention entry points validate their arguments before any device work: every case here returns PRL_EINVAL and a
message on a machine without a GPU (the pointers are never followed), and an empty batch is a no-op."""

import ctypes

import pytest

from pipelinerl_amd import _lib
from pipelinerl_amd.fused_attention import varlen_attention  # noqa: F401  (the feature these entry points belong to)

P = 0x10000  # a non-null, 16-byte aligned address that no case gets far enough to read


def fwd_args(**kw):
    a = dict(n=128, hq=4, hkv=2, d=64, q=P, qst=256, qsh=64, k=P, kst=128, ksh=64, v=P, vst=128, vsh=64, scale=0.125, ss=P, se=P, out=P, lse=P)
    a.update(kw)
    return [a[x] for x in ("n", "hq", "hkv", "d", "q", "qst", "qsh", "k", "kst", "ksh", "v", "vst", "vsh", "scale", "ss", "se", "out", "lse")] + [None]


def bwd_args(**kw):
    a = dict(n=128, hq=4, hkv=2, d=64, q=P, qst=256, qsh=64, k=P, kst=128, ksh=64, v=P, vst=128, vsh=64, scale=0.125, ss=P, se=P, out=P, lse=P, g=P,
             dq=P, dk=P, dv=P, ws=P, ws_bytes=1 << 20)
    a.update(kw)
    return [a[x] for x in ("n", "hq", "hkv", "d", "q", "qst", "qsh", "k", "kst", "ksh", "v", "vst", "vsh", "scale", "ss", "se", "out", "lse", "g", "dq",
                           "dk", "dv", "ws", "ws_bytes")] + [None]


BAD = {
    "negative_n": (dict(n=-1), b"negative"),
    "head_size_96": (dict(d=96), b"head size"),
    "head_size_0": (dict(d=0), b"head size"),
    "hq_not_multiple_of_hkv": (dict(hq=3, hkv=2), b"multiple"),
    "no_heads": (dict(hq=0), b"positive"),
    "negative_kv_heads": (dict(hkv=-2), b"positive"),
    "null_q": (dict(q=None), b"q is null"),
    "null_k": (dict(k=None), b"k is null"),
    "null_v": (dict(v=None), b"v is null"),
    "null_table": (dict(ss=None), b"null"),
    "null_lse": (dict(lse=None), b"null"),
    "null_out": (dict(out=None), b"out"),
    "q_token_stride_breaks_alignment": (dict(qst=260), b"alignment"),
    "k_head_stride_breaks_alignment": (dict(ksh=68), b"alignment"),
    "v_token_stride_below_d": (dict(vst=32), b"stride"),
    "q_pointer_unaligned": (dict(q=P + 2), b"aligned"),
}


@pytest.mark.parametrize("name", list(BAD))
def test_forward_rejects(libprl, name):
    kw, word = BAD[name]
    assert libprl.prl_attn_varlen_fwd(*fwd_args(**kw)) == _lib.PRL_EINVAL
    assert word in libprl.prl_last_error(), libprl.prl_last_error()


@pytest.mark.parametrize("name", list(BAD))
def test_backward_rejects(libprl, name):
    kw, word = BAD[name]
    assert libprl.prl_attn_varlen_bwd(*bwd_args(**kw)) == _lib.PRL_EINVAL
    assert word in libprl.prl_last_error(), libprl.prl_last_error()


def test_backward_rejects_its_own_arguments(libprl):
    need = ctypes.c_size_t(0)
    assert libprl.prl_attn_workspace_bytes(128, 4, ctypes.byref(need)) == 0
    for kw, word in ((dict(ws_bytes=need.value - 1), b"too small"), (dict(ws=None), b"workspace"), (dict(ws=P + 4), b"workspace"),
                     (dict(g=None), b"null"), (dict(dq=None), b"null"), (dict(dk=None), b"null"), (dict(dv=None), b"null"), (dict(dv=P + 8), b"aligned")):
        assert libprl.prl_attn_varlen_bwd(*bwd_args(**kw)) == _lib.PRL_EINVAL, kw
        assert word in libprl.prl_last_error(), (kw, libprl.prl_last_error())


def test_empty_batch_is_a_no_op(libprl):
    assert libprl.prl_attn_varlen_fwd(*fwd_args(n=0, q=None, k=None, v=None, out=None, lse=None, ss=None, se=None)) == 0
    assert libprl.prl_attn_varlen_bwd(*bwd_args(n=0, q=None, g=None, dq=None, ws=None, ws_bytes=0)) == 0
    assert libprl.prl_attn_segments(0, 16, None, None, 0, None, None, None) == 0
    assert libprl.prl_attn_segments(4, 0, None, None, 0, None, None, None) == 0
    assert libprl.prl_attn_varlen_fwd(*fwd_args(n=0, d=96)) == _lib.PRL_EINVAL  # ... but still a checked call


def test_segments_rejects(libprl):
    for args, word in (((-1, 8, None, None, 0, P, P, None), b"negative"), ((2, -8, None, None, 0, P, P, None), b"negative"),
                       ((1 << 20, 1 << 20, None, None, 0, P, P, None), b"int32"), ((2, 8, None, P, 2, P, P, None), b"mask_elem_bytes"),
                       ((2, 8, None, None, 0, None, P, None), b"null"), ((2, 8, P, None, 0, P, None, None), b"null")):
        assert libprl.prl_attn_segments(*args) == _lib.PRL_EINVAL, args
        assert word in libprl.prl_last_error(), (args, libprl.prl_last_error())


def test_workspace_bytes(libprl):
    need = ctypes.c_size_t(0)
    assert libprl.prl_attn_workspace_bytes(128, 4, None) == _lib.PRL_EINVAL and b"null" in libprl.prl_last_error()
    assert libprl.prl_attn_workspace_bytes(-1, 4, ctypes.byref(need)) == _lib.PRL_EINVAL
    assert libprl.prl_attn_workspace_bytes(128, 0, ctypes.byref(need)) == _lib.PRL_EINVAL
    sizes = {}
    for n in (1, 63, 64, 65, 1000, 8192):
        for hq in (1, 4, 14, 28):
            assert libprl.prl_attn_workspace_bytes(n, hq, ctypes.byref(need)) == 0
            sizes[(n, hq)] = need.value
            assert need.value >= 4 * n * hq and need.value % 16 == 0  # delta [hq, n] in fp32: linear in n, nothing of size n x n
    for (n, hq), b in sizes.items():
        assert b > 0
        assert all(b <= b2 for (n2, hq2), b2 in sizes.items() if n2 >= n and hq2 >= hq)
    assert sizes[(8192, 28)] < 4 * 8192 * 28 + 16
