"""Generates tests/golden/nb12_small.npz by EXECUTING THE REFERENCE'S OWN SOURCE on the CPU: the code cell of
notebooks/12_just_3d_conv.ipynb of the reference checkout (REF of make_conv3d_golden.py) that defines `LitAutoEncoder`
(STRIDE, CHANNELS, N_HIST_IMAGES, KERNEL and the class), exec'd as written.  pytorch_lightning.LightningModule is the stub of
make_conv3d_golden.py (torch.nn.Module + a recording log_dict).  The cell names no device, so nothing of it is altered.

Run where the reference checkout is (it does not travel to the GPU box):   python tests/golden/make_nb12_golden.py

Inputs and initial parameters are drawn from seeds by draw_batch / draw_parameters below (which the tests import), so the
fixture holds results only: y_hat, the three losses, the step-0 gradients and the parameters after three Adam steps of
  a/  H = W = 23, B = 3, horizons of 1, 9 and 23 timesteps (normalised as the notebook's loader does: -1.66, -0.51, 1.52)
  b/  H = 12, W = 38, B = 2, horizons of 12 and 24 timesteps (-0.07, 1.66); non-square
Seeds.  As make_nb10_golden.py explains, Adam's first step is lr * g / (|g| + eps), so an entry whose gradient is within
rounding of 0 moves by anything in +-lr, and a ReLU unit whose pre-activation is within rounding of 0 may be gated either way
by two correct implementations.  check_fit keeps both knives: it runs the same three steps in float64
(tests/nb12_reference.py) and refuses a fixture whose float32 parameters are not within FIT_Q99 of them at the 99th
percentile of every tensor, FIT_Q99 = 1e-7 being a tenth of the 1e-6 the tests ask of the kernels (the notebook's lr is 1e-4,
a tenth of notebook 10's, and so is every figure of the three-step rule); and it asks, before each of the three float64
steps, that every unit's |pre-activation| exceeds FIT_RELU_MARGIN = 3e-8 of its sum of |products|.  Each case's seed is the
first from 1001 (a) / 1002 (b) up that passes both (a: 1009, after eight draws with a ReLU unit inside the margin; b: 1002).
Both criteria involve the reference and float64 only, never the kernels under test.
A tensor above 20 000 elements is stored as 4 096 seeded entries (sample_index) plus its float64 sum and norm.
"""
import json
import os
import sys
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

OUT = os.path.join(HERE, "nb12_small.npz")
KEYS = ("FORECAST_HORIZON", "HISTORICAL_SAT_IMAGES", "TARGET_SAT_IMAGE")
CASES = {"a": dict(h=23, w=23, timesteps=(1, 9, 23), seed=1009), "b": dict(h=12, w=38, timesteps=(12, 24), seed=1002)}
LR = 1e-4           # the notebook's configure_optimizers
FIT_Q99 = 1e-7      # see check_fit
FIT_RELU_MARGIN = 0.03 * 1e-6      # ... of a unit's sum of |products|
PARAM_SHAPES = {"conv.0.weight": (64, 2, 2, 3, 3), "conv.0.bias": (64,), "conv.2.weight": (128, 64, 2, 3, 3),
                "conv.2.bias": (128,), "conv.4.weight": (128, 128, 2, 3, 3), "conv.4.bias": (128,),
                "conv.6.weight": (128, 128, 2, 3, 3), "conv.6.bias": (128,), "conv.8.weight": (1, 128, 2, 3, 3),
                "conv.8.bias": (1,)}
SAMPLE_ABOVE, N_SAMPLE = 20000, 4096


def out_side(s):
    return (s - 1) // 2 + 1


def normalise_forecast_horizon(timesteps):
    """12_just_3d_conv.ipynb:757-768: float32 (h - mean) / std of arange(1, 25)."""
    seq = np.arange(1, 25, dtype=np.float32)
    h = np.float32(timesteps)
    h -= seq.mean()
    h /= seq.std()
    return h


def draw_batch(tag, seed=None):
    """The case's batch: normalised-looking history and target (N(0, 1)), the horizons as the loader's float32."""
    c = CASES[tag]
    g = torch.Generator().manual_seed(c["seed"] if seed is None else seed)
    b = len(c["timesteps"])
    return {"HISTORICAL_SAT_IMAGES": torch.randn(b, 4, c["h"], c["w"], generator=g),
            "FORECAST_HORIZON": torch.tensor([normalise_forecast_horizon(t) for t in c["timesteps"]], dtype=torch.float32),
            "TARGET_SAT_IMAGE": torch.randn(b, out_side(c["h"]), out_side(c["w"]), generator=g)}


def draw_parameters(seed=1000):
    """The initial state_dict: uniform in +-1 / sqrt(fan_in), the range of nn.Conv3d's own initialisation."""
    g = torch.Generator().manual_seed(seed)
    state = {}
    for k, shape in PARAM_SHAPES.items():
        fan_in = int(np.prod(PARAM_SHAPES[k.replace("bias", "weight")][1:]))
        state[k] = (torch.rand(*shape, generator=g) * 2 - 1) * fan_in ** -0.5
    return state


def sample_index(name, numel):
    """Flat indices of the stored entries of tensor `name`: all of a small one, 4 096 seeded ones of a large one."""
    if numel <= SAMPLE_ABOVE:
        return None
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    return np.sort(rng.choice(numel, N_SAMPLE, replace=False))


def store(out, name, t):
    t = t.detach()
    idx = sample_index(name, t.numel())
    if idx is None:
        out[name] = t.numpy().copy()
        return
    out[name] = t.flatten()[torch.from_numpy(idx)].numpy().copy()
    out[name + "/sum"] = np.array(t.double().sum().item())
    out[name + "/norm"] = np.array(t.double().norm().item())


def load_notebook_class():
    from make_conv3d_golden import REF, install_stubs
    install_stubs()
    import pytorch_lightning as pl
    import torch.nn.functional as F
    from torch import nn
    path = os.path.join(REF, "notebooks", "12_just_3d_conv.ipynb")
    cells = ["".join(c["source"]) for c in json.load(open(path))["cells"] if c["cell_type"] == "code"]
    (class_src,) = [c for c in cells if "class LitAutoEncoder" in c]
    ns = dict(torch=torch, nn=nn, F=F, pl=pl, **{k: k for k in KEYS})
    exec(compile(class_src, path, "exec"), ns)
    return ns["LitAutoEncoder"]


def case(out, LitAutoEncoder, tag, seed=None):
    model = LitAutoEncoder()
    model.load_state_dict(draw_parameters())
    batch = draw_batch(tag, seed)
    store(out, f"{tag}/y_hat", model(batch))
    opt = model.configure_optimizers()
    assert opt.param_groups[0]["lr"] == LR
    losses = []
    for step in range(3):
        opt.zero_grad()
        loss = model.training_step(batch, 0)
        loss.backward()
        if step == 0:
            for k, p in model.named_parameters():
                store(out, f"{tag}/grad/{k}", p.grad)
        opt.step()
        losses.append(float(loss.detach()))
    for k, p in model.named_parameters():
        store(out, f"{tag}/step3/{k}", p)
    out[f"{tag}/losses"] = np.array(losses)
    check_fit(tag, model, seed)


def check_fit(tag, model, seed=None):
    """The notebook model's float32 parameters after its three steps against the same steps in float64."""
    sys.path.insert(0, os.path.dirname(HERE))
    import nb12_reference as R
    batch = draw_batch(tag, seed)
    p = R.params64(draw_parameters())
    opt = torch.optim.Adam(list(p.values()), lr=LR)
    for step in range(3):
        margin = R.relu_margin64(p, batch, FIT_RELU_MARGIN)
        assert margin > 1.0, f"case {tag}: a ReLU unit within {margin:.2f} x the rounding margin of 0 at step {step}; draw another seed"
        opt.zero_grad()
        R.loss64(R.forward64(p, batch), batch["TARGET_SAT_IMAGE"]).backward()
        opt.step()
    for k, v in model.named_parameters():
        err = (v.detach().double() - p[k].detach()).abs().flatten().sort().values
        q99 = err[int(0.99 * (err.numel() - 1))].item()
        assert q99 <= FIT_Q99, f"case {tag}: {k} differs from float64 by {q99:.2e} at the 99th percentile; draw another seed"


def main():
    LitAutoEncoder = load_notebook_class()
    out = {}
    for tag in CASES:
        case(out, LitAutoEncoder, tag)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT) // 1024, "KiB;", len(out), "arrays")


if __name__ == "__main__":
    main()
