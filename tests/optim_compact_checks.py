"""Reference side of the compact optimizer step (csrc/prl_optim_sr.h, csrc/prl_optim_compact.hip), in numpy.

The rounding rule restated independently of the header: Philox4x32-10, the call indexing, the three 16-bit values cut from a word,
stochastic rounding and round-to-nearest-even of fp32 to bf16.  And the COMPOSITION ORACLE of one compact step:
  widen (numpy)  ->  `prl_host_adamw` / `prl_host_lion` of tests/harness/optim_math_host.cpp, which tests/test_optim_math_host.py
  pins to torch.optim.AdamW and to the golden record of the reference's Lion  ->  numpy `sr` with numpy Philox.
Nothing of csrc/prl_optim_sr.h enters the oracle, so the header (tests/test_optim_compact_host.py) and the kernel
(tests/test_gpu_optim_compact.py) are both compared with something they do not contain.

Entry classification against a device (`classify`): the GPU's sqrt and divide may differ from the host's in the last fp32 ulps, so
the value a store rounds may be a few ulp from the oracle's.  A bf16 store of the oracle's pre-rounding bits u with the 16-bit
addend a (the random value; for round-to-nearest-even 0x7fff + bit 16 of u) is DECIDED when (u & 0xffff) + a is not within 4 of
65536: then no value within 4 ulp of u rounds differently, and the stored bf16 must be bit-equal.  Otherwise it must be one of the
two bf16 neighbours of the oracle's value.  For a uniform addend at most 8 of 65536 values are undecided, whatever the kernel does."""

from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
F = ctypes.POINTER(ctypes.c_float)
D = ctypes.c_double

KNOWN_ANSWERS = [  # (counter, key, output) of Philox4x32-10
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]
UNDECIDED_MARGIN = 4  # fp32 ulps the device's pre-rounding value may be away from the oracle's


# ---- the rounding rule ------------------------------------------------------------------------------------------------
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Vectorised over the counter words (uint32 arrays or ints); returns the four output words as uint32 arrays."""
    mask = np.uint64(0xFFFFFFFF)
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) & mask for x in (c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]  # < 2^64: exact
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & mask]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    shape = np.broadcast(*c).shape
    return [np.broadcast_to(x, shape).astype(np.uint32) for x in c]


def sr_words(index, step: int, ordinal: int, seed: int) -> np.ndarray:
    """The output word of every element: `index` = indices INSIDE THE PARAMETER.  counter = (q lo, q hi, step, ordinal) with q = index // 4,
    key = (seed lo, seed hi); element 4q + j takes word j."""
    index = np.asarray(index, dtype=np.int64)
    q = index >> 2
    words = philox4x32_10(q & 0xFFFFFFFF, q >> 32, step & 0xFFFFFFFF, ordinal, seed & 0xFFFFFFFF, seed >> 32)
    return np.choose(index & 3, words).astype(np.uint32)


def r_p(x):
    return np.asarray(x, dtype=np.uint32) & np.uint32(0xFFFF)


def r_m(x):
    return np.asarray(x, dtype=np.uint32) >> np.uint32(16)


def r_v(x):
    return r_p(x) ^ r_m(x)


def bits32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def widen(h) -> np.ndarray:
    """bf16 bit patterns (uint16) -> fp32, exact."""
    return (np.ascontiguousarray(h, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def _nan(u):
    return (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def sr(f, r) -> np.ndarray:
    """fp32 -> bf16 bits: (bits + r) >> 16, NaN -> 0x7FC0."""
    u = bits32(f)
    out = ((u.astype(np.uint64) + np.asarray(r, dtype=np.uint64)) >> np.uint64(16)).astype(np.uint16)
    return np.where(_nan(u), np.uint16(0x7FC0), out)


def rne_addend(f) -> np.ndarray:
    """Round-to-nearest-even written as an addend: 0x7fff + bit 16."""
    u = bits32(f)
    return np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))


def rne(f) -> np.ndarray:
    return sr(f, rne_addend(f))


def to_bf16_bits(a) -> np.ndarray:
    """fp32 values that ARE bf16-representable -> their bit patterns."""
    u = bits32(a)
    assert not np.any(u & np.uint32(0xFFFF)), "not bf16-representable"
    return (u >> np.uint32(16)).astype(np.uint16)


# ---- the harnesses ----------------------------------------------------------------------------------------------------
def _compile(src: str, out: Path) -> ctypes.CDLL:
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", f"-I{ROOT / 'include'}", "-o", str(out), str(ROOT / "tests" / "harness" / src)])
    return ctypes.CDLL(str(out))


def build_optmath(tmpdir: Path) -> ctypes.CDLL:
    """tests/harness/optim_math_host.cpp: the fp32 updates the parent pins to torch and the Lion golden."""
    lib = _compile("optim_math_host.cpp", Path(tmpdir) / "liboptmath.so")
    lib.prl_host_adamw.restype = None
    lib.prl_host_adamw.argtypes = [ctypes.c_long, D, D, D, D, D, ctypes.c_long, ctypes.c_float, F, F, F, F]
    lib.prl_host_lion.restype = None
    lib.prl_host_lion.argtypes = [ctypes.c_long, D, D, D, D, ctypes.c_float, F, F, F]
    return lib


def build_compact(tmpdir: Path) -> ctypes.CDLL:
    """tests/harness/optim_compact_host.cpp: csrc/prl_optim_sr.h compiled for the host."""
    lib = _compile("optim_compact_host.cpp", Path(tmpdir) / "liboptcompact.so")
    U32, V = ctypes.POINTER(ctypes.c_uint32), ctypes.c_void_p
    lib.prl_host_philox4x32_10.restype = None
    lib.prl_host_philox4x32_10.argtypes = [U32, U32, U32]
    lib.prl_host_sr_words.restype = None
    lib.prl_host_sr_words.argtypes = [ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_uint64, U32]
    lib.prl_host_sr.restype = ctypes.c_uint16
    lib.prl_host_sr.argtypes = [ctypes.c_float, ctypes.c_uint32]
    lib.prl_host_sr_all.restype = None
    lib.prl_host_sr_all.argtypes = [ctypes.c_float, ctypes.POINTER(ctypes.c_uint16)]
    lib.prl_host_compact_adamw.restype = None
    lib.prl_host_compact_adamw.argtypes = [ctypes.c_long, D, D, D, D, D, ctypes.c_long, ctypes.c_float, F, V, F, V, V, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_long, ctypes.c_long, ctypes.c_uint64]
    lib.prl_host_compact_lion.restype = None
    lib.prl_host_compact_lion.argtypes = [ctypes.c_long, D, D, D, D, ctypes.c_long, ctypes.c_float, F, V, F, V, ctypes.c_int, ctypes.c_int, ctypes.c_long,
                                          ctypes.c_long, ctypes.c_uint64]
    return lib


def fp(a):
    return a.ctypes.data_as(F)


# ---- the composition oracle ---------------------------------------------------------------------------------------------
MODES = ("f32", "master", "nearest", "stochastic")  # = param_mode 0 .. 3 of the harness and the kernel


class Stored:
    """One stored array of a step: `pre` the fp32 value before the store, `addend` what the store adds to its bits before cutting
    them (None: stored as fp32, exactly), `out` what is stored (fp32 values, or bf16 bits as uint16)."""

    def __init__(self, pre, addend, out):
        self.pre, self.addend, self.out = pre, addend, out


class CompactOracle:
    """State of ONE parameter (or piece) and the compact step on it.  `p`: fp32 values (mode "f32") or bf16 bits (uint16);
    `master`: fp32 (mode "master"); `m`, `v`: fp32 values or bf16 bits by `state_bf16`; `v` None for Lion."""

    def __init__(self, optmath, rule: str, mode: str, state_bf16: bool, p, m=None, v=None, master=None, *, lr, wd, betas, eps=1e-8, seed=0, ordinal=0,
                 elem_offset=0):
        assert rule in ("adamw", "lion") and mode in MODES
        self.lib, self.rule, self.mode, self.sb = optmath, rule, mode, bool(state_bf16)
        self.lr, self.wd, self.betas, self.eps, self.seed, self.ordinal, self.elem_offset = lr, wd, betas, eps, seed, ordinal, elem_offset
        self.p = np.array(p, dtype=np.float32 if mode == "f32" else np.uint16)
        n = self.p.size
        sdt = np.uint16 if self.sb else np.float32
        self.m = np.zeros(n, sdt) if m is None else np.array(m, dtype=sdt)
        self.v = None if rule == "lion" else (np.zeros(n, sdt) if v is None else np.array(v, dtype=sdt))
        self.master = None
        if mode == "master":
            self.master = widen(self.p).copy() if master is None else np.array(master, dtype=np.float32)

    def _f32(self, a):
        return (widen(a) if a.dtype == np.uint16 else a).astype(np.float32).copy()

    def step(self, g, coef: float, step: int) -> dict[str, Stored]:
        """One update with gradient `g` (fp32 values as the device sees them); returns what was stored, by array name."""
        n = self.p.size
        g = np.ascontiguousarray(g, dtype=np.float32)
        w = self.master.copy() if self.mode == "master" else self._f32(self.p)
        m32 = self._f32(self.m)
        b1, b2 = self.betas
        if self.rule == "adamw":
            v32 = self._f32(self.v)
            self.lib.prl_host_adamw(n, self.lr, self.wd, b1, b2, self.eps, step, np.float32(coef), fp(g), fp(w), fp(m32), fp(v32))
        else:
            self.lib.prl_host_lion(n, self.lr, self.wd, b1, b2, np.float32(coef), fp(g), fp(w), fp(m32))
        x = sr_words(self.elem_offset + np.arange(n, dtype=np.int64), step, self.ordinal, self.seed)
        out = {}

        def state(pre, addend):
            return Stored(pre, addend, sr(pre, addend)) if self.sb else Stored(pre, None, pre)

        out["exp_avg"] = state(m32, r_m(x))
        self.m = out["exp_avg"].out
        if self.rule == "adamw":
            out["exp_avg_sq"] = state(v32, r_v(x))
            self.v = out["exp_avg_sq"].out
        if self.mode == "f32":
            out["param"] = Stored(w, None, w)
        else:
            addend = r_p(x) if self.mode == "stochastic" else rne_addend(w)
            out["param"] = Stored(w, addend, sr(w, addend))
            if self.mode == "master":
                out["master"] = Stored(w, None, w)
                self.master = w
        self.p = out["param"].out
        return out


def classify(stored: Stored):
    """(decided mask, lower neighbour, upper neighbour) of a bf16 store: module docstring."""
    u = bits32(stored.pre)
    s = (u & np.uint32(0xFFFF)).astype(np.int64) + np.asarray(stored.addend, dtype=np.int64)
    decided = np.abs(s - 65536) > UNDECIDED_MARGIN
    lo = (u >> np.uint32(16)).astype(np.uint16)
    return decided | _nan(u), lo, (lo + np.uint16(1)).astype(np.uint16)


def check_store(name: str, got, stored: Stored, edge=None) -> tuple[int, int]:
    """Assert one stored array of the device against the oracle's.  bf16: decided entries bit-equal, undecided ones one of the two
    neighbours.  fp32: within UNDECIDED_MARGIN ulp (the same allowance for the device's sqrt and divide; 0 observed is printed).
    `edge`: boolean mask of entries reported separately.  Returns (entries, undecided or inexact entries)."""
    got = np.ascontiguousarray(got).ravel()
    n = got.size
    edge = np.zeros(n, dtype=bool) if edge is None else edge
    if stored.addend is None:
        a, b = bits32(got).astype(np.int64), bits32(stored.out).astype(np.int64)
        same_sign = (a >> 31) == (b >> 31)
        dist = np.where(same_sign, np.abs(a - b), (a & 0x7FFFFFFF) + (b & 0x7FFFFFFF))
        nan_ok = np.isnan(got) & np.isnan(stored.out)
        bad = (dist > UNDECIDED_MARGIN) & ~nan_ok
        inexact = int(((dist != 0) & ~nan_ok).sum())
        print(f"[compact] {name}: fp32, {n} entries, {inexact} not bit-equal (max {int(dist.max(initial=0))} ulp), edges: {int(edge.sum())} entries, "
              f"{int(((dist != 0) & ~nan_ok & edge).sum())} not bit-equal")
        assert not bad.any(), f"{name}: entry {int(np.argmax(bad))} is {int(dist[np.argmax(bad)])} ulp from the oracle"
        return n, inexact
    assert got.dtype == np.uint16
    decided, lo, hi = classify(stored)
    equal = got == stored.out
    neighbour = (got == lo) | (got == hi)
    wrong = (decided & ~equal) | (~decided & ~neighbour)
    print(f"[compact] {name}: bf16, {n} entries, {int((~decided).sum())} undecided, {int((~equal).sum())} not bit-equal; edges: {int(edge.sum())} entries, "
          f"{int((~decided & edge).sum())} undecided, {int((wrong & edge).sum())} wrong")
    # 2 x 4 + 1 of the 65536 addends leave an entry undecided; 4 x that share (and 8 entries) is far outside chance on random data
    assert (~decided).sum() <= max(8, 4 * n * (2 * UNDECIDED_MARGIN + 1) / 65536), f"{name}: too many undecided entries for the comparison to mean much"
    assert not wrong.any(), (f"{name}: entry {int(np.argmax(wrong))}: got {int(got[np.argmax(wrong)]):#06x}, oracle {int(stored.out[np.argmax(wrong)]):#06x} "
                             f"(decided: {bool(decided[np.argmax(wrong)])})")
    return n, int((~decided).sum())


# ---- the unbiasedness experiments ---------------------------------------------------------------------------------------
DRIFT = dict(n=65536, steps=200, lr=1e-5, p0=1.0, g=1.0)
DECAY = dict(n=65536, steps=200, v0=1.0, beta2=0.999)
SE_MARGIN = 4.0  # standard errors


def adamw_witness_fp64(p0: float, g: float, lr: float, steps: int, betas=(0.9, 0.999), eps=1e-8) -> float:
    """AdamW without decay on one fp64 scalar with a constant gradient."""
    p = m = v = 0.0
    p = float(p0)
    for t in range(1, steps + 1):
        m = betas[0] * m + (1 - betas[0]) * g
        v = betas[1] * v + (1 - betas[1]) * g * g
        p -= lr / (1 - betas[0] ** t) * m / ((v ** 0.5) / ((1 - betas[1] ** t) ** 0.5) + eps)
    return p


def assert_within_standard_errors(name: str, values, expected: float) -> float:
    values = np.asarray(values, dtype=np.float64)
    se = values.std() / np.sqrt(values.size)
    z = abs(values.mean() - expected) / se if se > 0 else (0.0 if values.mean() == expected else np.inf)
    print(f"[compact] {name}: mean {values.mean():.8f}, expected {expected:.8f}, std {values.std():.3e}, {z:.2f} standard errors (bound {SE_MARGIN})")
    assert se > 0, f"{name}: no entry moved"
    assert z <= SE_MARGIN, f"{name}: {z:.2f} standard errors from the expectation"
    return z
