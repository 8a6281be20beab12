"""The slice-form attention entry points validate their arguments before any device work: every case here returns PRL_EINVAL and
a message on a machine without a GPU (the pointers are never followed), and an empty slice is a no-op."""

import ctypes

import pytest

from pipelinerl_amd import _lib
from pipelinerl_amd.fused_attention import varlen_attention_slice  # noqa: F401  (the feature these entry points belong to)

P = 0x10000  # a non-null, 16-byte aligned address that no case gets far enough to read

FWD = ("nq", "nk", "q_off", "hq", "hkv", "d", "q", "qst", "qsh", "k", "kst", "ksh", "v", "vst", "vsh", "scale", "ss", "se", "out", "lse")
BWD = FWD + ("g", "dq", "dk", "dv", "ws", "ws_bytes")


def args(names, **kw):
    a = dict(nq=96, nk=384, q_off=96, hq=4, hkv=2, d=64, q=P, qst=256, qsh=64, k=P, kst=128, ksh=64, v=P, vst=128, vsh=64, scale=0.125, ss=P, se=P,
             out=P, lse=P, g=P, dq=P, dk=P, dv=P, ws=P, ws_bytes=1 << 20)
    a.update(kw)
    return [a[x] for x in names] + [None]


BAD = {
    "negative_nq": (dict(nq=-1), b"negative"),
    "negative_nk": (dict(nk=-1), b"negative"),
    "head_size_96": (dict(d=96), b"head size"),
    "head_size_0": (dict(d=0), b"head size"),
    "hq_not_multiple_of_hkv": (dict(hq=3, hkv=2), b"multiple"),
    "no_heads": (dict(hq=0), b"positive"),
    "negative_kv_heads": (dict(hkv=-2), b"positive"),
    "negative_offset": (dict(q_off=-1), b"q_off"),
    "offset_past_the_row": (dict(q_off=289), b"q_off"),
    "more_queries_than_keys": (dict(nq=385, q_off=0), b"q_off"),
    "offset_overflows": (dict(q_off=(1 << 63) - 1), b"q_off"),
    "null_q": (dict(q=None), b"q is null"),
    "null_k": (dict(k=None), b"k is null"),
    "null_v": (dict(v=None), b"v is null"),
    "null_seq_start": (dict(ss=None), b"null"),
    "null_seq_end": (dict(se=None), b"null"),
    "null_lse": (dict(lse=None), b"null"),
    "null_out": (dict(out=None), b"out"),
    "q_token_stride_breaks_alignment": (dict(qst=260), b"alignment"),
    "q_head_stride_breaks_alignment": (dict(qsh=68), b"alignment"),
    "k_token_stride_breaks_alignment": (dict(kst=132), b"alignment"),
    "k_head_stride_breaks_alignment": (dict(ksh=68), b"alignment"),
    "v_token_stride_breaks_alignment": (dict(vst=132), b"alignment"),
    "v_token_stride_below_d": (dict(vst=32), b"stride"),
    "q_pointer_unaligned": (dict(q=P + 2), b"aligned"),
}


@pytest.mark.parametrize("name", list(BAD))
def test_forward_rejects(libprl, name):
    kw, word = BAD[name]
    assert libprl.prl_attn_slice_fwd(*args(FWD, **kw)) == _lib.PRL_EINVAL
    assert word in libprl.prl_last_error(), libprl.prl_last_error()


@pytest.mark.parametrize("name", list(BAD))
def test_backward_rejects(libprl, name):
    kw, word = BAD[name]
    assert libprl.prl_attn_slice_bwd(*args(BWD, **kw)) == _lib.PRL_EINVAL
    assert word in libprl.prl_last_error(), libprl.prl_last_error()


def test_backward_rejects_its_own_arguments(libprl):
    need = ctypes.c_size_t(0)
    assert libprl.prl_attn_slice_workspace_bytes(96, 4, ctypes.byref(need)) == 0
    for kw, word in ((dict(ws_bytes=need.value - 1), b"too small"), (dict(ws=None), b"workspace"), (dict(ws=P + 4), b"workspace"),
                     (dict(g=None), b"null"), (dict(dq=None), b"null"), (dict(dk=None), b"null"), (dict(dv=None), b"null"), (dict(dv=P + 8), b"aligned"),
                     (dict(dk=P + 4), b"aligned")):
        assert libprl.prl_attn_slice_bwd(*args(BWD, **kw)) == _lib.PRL_EINVAL, kw
        assert word in libprl.prl_last_error(), (kw, libprl.prl_last_error())


def test_the_edges_of_the_offset_range_are_accepted_as_far_as_validation_goes(libprl):
    """q_off = 0 and q_off + nq == nk pass the range check: the next check (a null q) is the one that answers."""
    for kw in (dict(q_off=0), dict(q_off=288), dict(nq=384, q_off=0)):
        assert libprl.prl_attn_slice_fwd(*args(FWD, q=None, **kw)) == _lib.PRL_EINVAL
        assert b"q is null" in libprl.prl_last_error(), (kw, libprl.prl_last_error())


def test_empty_slice_is_a_no_op(libprl):
    nothing = dict(nq=0, q=None, k=None, v=None, out=None, lse=None, ss=None, se=None)
    assert libprl.prl_attn_slice_fwd(*args(FWD, **nothing)) == 0
    assert libprl.prl_attn_slice_fwd(*args(FWD, q_off=384, **nothing)) == 0  # an empty slice at the end of the row
    assert libprl.prl_attn_slice_bwd(*args(BWD, g=None, dq=None, dk=None, dv=None, ws=None, ws_bytes=0, **nothing)) == 0
    assert libprl.prl_attn_slice_fwd(*args(FWD, d=96, **nothing)) == _lib.PRL_EINVAL  # ... but still a checked call
    assert libprl.prl_attn_slice_fwd(*args(FWD, q_off=385, **nothing)) == _lib.PRL_EINVAL and b"q_off" in libprl.prl_last_error()


def test_workspace_bytes(libprl):
    need = ctypes.c_size_t(0)
    assert libprl.prl_attn_slice_workspace_bytes(128, 4, None) == _lib.PRL_EINVAL and b"null" in libprl.prl_last_error()
    assert libprl.prl_attn_slice_workspace_bytes(-1, 4, ctypes.byref(need)) == _lib.PRL_EINVAL
    assert libprl.prl_attn_slice_workspace_bytes(128, 0, ctypes.byref(need)) == _lib.PRL_EINVAL
    for nq in (0, 1, 63, 64, 65, 129, 2048):
        for hq in (1, 4, 7, 28):
            assert libprl.prl_attn_slice_workspace_bytes(nq, hq, ctypes.byref(need)) == 0
            assert 4 * nq * hq <= need.value < 4 * nq * hq + 16 and need.value % 16 == 0  # delta [hq, nq] in fp32: the LOCAL rows only


def test_fold_rejects(libprl):
    for a, word in (((0, 64, P, P, None), b"P 0"), ((-3, 64, P, P, None), b"P -3"), ((2, -1, P, P, None), b"negative"),
                    ((2, 64, None, P, None), b"null"), ((2, 64, P, None, None), b"null"), ((2, 64, P + 4, P, None), b"aligned"),
                    ((2, 64, P, P + 2, None), b"aligned"), ((65535, 1 << 62, P, P, None), b"overflows"), ((1 << 20, 64, P, P, None), b"at most")):
        assert libprl.prl_attn_fold_parts(*a) == _lib.PRL_EINVAL, a
        assert word in libprl.prl_last_error(), (a, libprl.prl_last_error())
    assert libprl.prl_attn_fold_parts(3, 0, None, None, None) == 0  # nothing to fold
    assert libprl.prl_attn_fold_parts(0, 0, None, None, None) == _lib.PRL_EINVAL
