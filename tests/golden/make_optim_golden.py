"""Golden vectors for the Lion optimizer of the reference (pipelinerl/finetune/optim.py:48-112), produced by RUNNING the
reference's own `Lion` class for 5 steps on fp32 CPU tensors: two parameter groups (weight decay 0.01 / 0), momentum seeded
with N(0, 1), gradients of log-uniform scale 1e-6 ... 1.  Inputs and every step's `p` / `exp_avg` are recorded
(tests/golden/optim_lion.npz); only arrays are stored.

The module imports `peft`, which need not be installed: that one import is replaced by an empty stand-in at generation time.

    python tests/golden/make_optim_golden.py <path to a checkout of the reference>
"""

from __future__ import annotations

import importlib.util
import sys
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
STEPS = 5
SIZES = (517, 131)  # not multiples of the CPU vector width: torch's vector body AND its scalar tail are in the record
LR, BETAS, DECAYS = 1e-4, (0.9, 0.99), (0.01, 0.0)


def load_reference(root: Path):
    from transformers import Adafactor, PreTrainedModel  # noqa: F401  (first: transformers must probe for peft BEFORE the stand-in exists)

    if "peft" not in sys.modules:
        peft = types.ModuleType("peft")
        peft_model = types.ModuleType("peft.peft_model")
        peft_model.PeftModel = type("PeftModel", (), {})
        peft.peft_model = peft_model
        sys.modules["peft"], sys.modules["peft.peft_model"] = peft, peft_model
    spec = importlib.util.spec_from_file_location("reference_optim", root / "pipelinerl" / "finetune" / "optim.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main() -> None:
    ref = load_reference(Path(sys.argv[1]))
    rng = np.random.default_rng(2024)
    out: dict[str, np.ndarray] = {"lr": np.float64(LR), "betas": np.asarray(BETAS, np.float64), "weight_decay": np.asarray(DECAYS, np.float64)}
    params = [torch.nn.Parameter(torch.from_numpy(rng.normal(0.0, 0.05, n).astype(np.float32))) for n in SIZES]
    opt = ref.Lion([{"params": [p], "weight_decay": wd} for p, wd in zip(params, DECAYS)], lr=LR, betas=BETAS)
    for k, p in enumerate(params):
        m0 = rng.normal(0.0, 1.0, p.numel()).astype(np.float32)
        opt.state[p]["exp_avg"] = torch.from_numpy(m0.copy())
        out[f"g{k}/p0"], out[f"g{k}/m0"] = p.detach().numpy().copy(), m0
    for step in range(STEPS):
        for k, p in enumerate(params):
            scale = 10.0 ** rng.uniform(-6.0, 0.0, p.numel())
            g = (rng.normal(0.0, 1.0, p.numel()) * scale).astype(np.float32)
            m = opt.state[p]["exp_avg"].numpy()
            # the sign must be decided: no zero, and fp32 and fp64 agree on it
            u32 = m * np.float32(BETAS[0]) + g * np.float32(1 - BETAS[0])
            u64 = m.astype(np.float64) * BETAS[0] + g.astype(np.float64) * (1 - BETAS[0])
            assert np.all(u32 != 0) and np.all(np.sign(u32) == np.sign(u64)), "an undecided sign in the inputs: change the seed"
            assert np.all(np.abs(u64) > 1e-6 * (np.abs(m * BETAS[0]) + np.abs(g * (1 - BETAS[0])))), "a sign within rounding of zero"
            p.grad = torch.from_numpy(g.copy())
            out[f"g{k}/grad{step}"] = g
        opt.step()
        for k, p in enumerate(params):
            out[f"g{k}/p{step + 1}"] = p.detach().numpy().copy()
            out[f"g{k}/m{step + 1}"] = opt.state[p]["exp_avg"].numpy().copy()
    np.savez_compressed(HERE / "optim_lion.npz", **out)
    size = (HERE / "optim_lion.npz").stat().st_size
    assert size <= 64 << 10, size
    print("wrote", HERE / "optim_lion.npz", len(out), "arrays", size, "bytes")


if __name__ == "__main__":
    main()
