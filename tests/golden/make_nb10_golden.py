"""Generates tests/golden/nb10_small.npz and tests/golden/nb10_sampler.npz by EXECUTING THE REFERENCE'S OWN SOURCE on the CPU:
the code cells of notebooks/10_just_conv.ipynb of the reference checkout (REF below) that define `LitAutoEncoder` (STRIDE,
CHANNELS, N_HIST_IMAGES, STRIPE_WIDTH and the class) and, for the sampler fixture, `sample_squares` and
`super_batch_to_example`, exec'd as written.  pytorch_lightning.LightningModule is the stub of make_conv3d_golden.py
(torch.nn.Module + a recording log_dict).  The class cell allocates its stripe plane with torch.zeros(..., device='cuda');
in this generator only, the `torch` name the cell sees forwards everything to torch except that `zeros` drops the device
argument, so the plane lands on the CPU.  Nothing else of the cell is altered.

Run where the reference checkout is (it does not travel to the GPU box):   python tests/golden/make_nb10_golden.py

Inputs and initial parameters are drawn from seeds by draw_batch / draw_parameters below (which the tests import), so the
fixture holds results only: y_hat, the three losses, the step-0 gradients and the parameters after three Adam steps of
  a/  H = W = 47, B = 3, horizons 1, 9, 23: a stripe inside the image, one clipped at the right edge (columns 45, 46 of
      45..49) and an empty one (start 115 >= W)
  b/  H = 20, W = 54, B = 2, horizons 0, 10: the stripe at column 0 and one clipped at the edge (columns 50..53 of 50..54);
      non-square
Seeds.  Adam's first step is lr * g / (|g| + eps): an entry whose gradient is within rounding of 0 moves by anything in +-lr, and
with a few such entries the second and third gradients differ by 1e-3 relative between two correct implementations.  A draw
in which that happens cannot pin parameters after three steps, whatever computes them: torch float32 and torch float64 on the
CPU then disagree with EACH OTHER on more than 1 % of a tensor by over 1e-5 (seeds 1001, 1002, 1004, 1005 of case a: 99th
percentile 1.0e-5 .. 3.4e-5).  check_fit therefore runs the same three steps in float64 (tests/nb10_reference.py) and
refuses a fixture whose float32 parameters are not within FIT_Q99 = 1e-6 of them at the 99th percentile of every tensor, a
tenth of what the tests ask of the kernels.  ReLU gates are the second knife edge: a unit whose pre-activation is within
float32 rounding of 0 may be gated either way by two correct implementations, and ONE such unit among the case's ~2 million
moves every gradient below it by about 1 / sqrt(units) of its norm, 1e-3 (seen with seed 1006 of case a).  check_fit
therefore also asks, before each of the three float64 steps, that every unit's |pre-activation| exceeds FIT_RELU_MARGIN =
3e-8 of its sum of |products|: ten times the expected rounding error u sum|p| / sqrt(K) of a float32 sum of K ~ 10^3 terms
(u = 6e-8).  Each case's seed is the first from 1001 (a) / 1002 (b) up that passes both (a: 1009, b: 1003; 99th percentiles
1.5e-8 and 1.4e-8).  Both criteria involve the reference and float64 only, never the kernels under test.
A tensor above 20 000 elements is stored as 4 096 seeded entries (sample_index) plus its float64 sum and norm.
The sampler fixture holds, for one seeded generator, the (hist_start, horizon, top, left) of N_DRAWS examples.
"""
import json
import os
import sys
import types
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

OUT = os.path.join(HERE, "nb10_small.npz")
OUT_SAMPLER = os.path.join(HERE, "nb10_sampler.npz")
KEYS = ("FORECAST_HORIZON", "HISTORICAL_SAT_IMAGES", "TARGET_SAT_IMAGE")
CASES = {"a": dict(h=47, w=47, horizons=(1, 9, 23), seed=1009), "b": dict(h=20, w=54, horizons=(0, 10), seed=1003)}
FIT_Q99 = 1e-6      # see check_fit
FIT_RELU_MARGIN = 0.03 * 1e-6      # ... of a unit's sum of |products|
PARAM_SHAPES = {"conv.0.weight": (64, 5, 3, 3), "conv.0.bias": (64,), "conv.2.weight": (128, 64, 3, 3), "conv.2.bias": (128,),
                "conv.4.weight": (128, 128, 3, 3), "conv.4.bias": (128,), "conv.6.weight": (1, 128, 3, 3), "conv.6.bias": (1,)}
SAMPLE_ABOVE, N_SAMPLE = 20000, 4096
N_DRAWS, SAMPLER_SEED, SAMPLER_SHAPE = 40, 42, (30, 150, 170)


def out_side(s):
    return (s - 1) // 2 + 1


def draw_batch(tag):
    """The case's batch: normalised-looking history and target (N(0, 1)), the horizons as int64."""
    c = CASES[tag]
    g = torch.Generator().manual_seed(c["seed"])
    b = len(c["horizons"])
    return {"HISTORICAL_SAT_IMAGES": torch.randn(b, 4, c["h"], c["w"], generator=g),
            "FORECAST_HORIZON": torch.tensor(c["horizons"], dtype=torch.int64),
            "TARGET_SAT_IMAGE": torch.randn(b, out_side(c["h"]), out_side(c["w"]), generator=g)}


def draw_parameters(seed=1000):
    """The initial state_dict: uniform in +-1 / sqrt(fan_in), the range of nn.Conv2d's own initialisation."""
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


def _notebook_cells():
    from make_conv3d_golden import REF
    path = os.path.join(REF, "notebooks", "10_just_conv.ipynb")
    nb = json.load(open(path))
    return path, ["".join(c["source"]) for c in nb["cells"] if c["cell_type"] == "code"]


def load_notebook_class():
    from make_conv3d_golden import install_stubs
    install_stubs()
    import pytorch_lightning as pl
    import torch.nn.functional as F
    from torch import nn

    class _TorchOnCpu(types.ModuleType):
        def __getattr__(self, name):
            return getattr(torch, name)

        @staticmethod
        def zeros(*args, device=None, **kw):
            return torch.zeros(*args, **kw)

    path, cells = _notebook_cells()
    (class_src,) = [c for c in cells if "class LitAutoEncoder" in c]
    ns = dict(torch=_TorchOnCpu("torch"), nn=nn, F=F, pl=pl, **{k: k for k in KEYS})
    exec(compile(class_src, path, "exec"), ns)
    return ns["LitAutoEncoder"]


def case(out, LitAutoEncoder, tag):
    model = LitAutoEncoder()
    model.load_state_dict(draw_parameters())
    batch = draw_batch(tag)
    store(out, f"{tag}/y_hat", model(batch))
    opt = model.configure_optimizers()
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
    check_fit(tag, model)


def check_fit(tag, model):
    """The notebook model's float32 parameters after its three steps against the same steps in float64."""
    sys.path.insert(0, os.path.dirname(HERE))
    import nb10_reference as R
    batch = draw_batch(tag)
    p = R.params64(draw_parameters())
    opt = torch.optim.Adam(list(p.values()), lr=0.001)
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


class _Values:
    def __init__(self, v):
        self.values = v


class _Frames:
    """What the sampler cells need of xr.DataArray(dims=(time, y, x)): len and .isel(time=...).values."""

    def __init__(self, data):
        self.data = data

    def __len__(self):
        return len(self.data)

    def isel(self, time):
        return _Values(self.data[time])


def sampler_frames():
    """[T, H, W] frames whose pixel (t, r, c) encodes its own position, so a crop names where it was taken."""
    t, h, w = SAMPLER_SHAPE
    return (np.arange(t, dtype=np.float64)[:, None, None] * 1e6 + np.arange(h, dtype=np.float64)[None, :, None] * 1e3
            + np.arange(w, dtype=np.float64)[None, None, :])


def sampler(out):
    from typing import Dict, Optional
    path, cells = _notebook_cells()
    ns = dict(np=np, Dict=Dict, Optional=Optional, SAT_IMAGES="SAT_IMAGES", **{k: k for k in KEYS})
    for marker in ("def sample_squares", "def super_batch_to_example"):
        src = [c for c in cells if c.lstrip().startswith(marker)][-1]      # the current definition, not the '''old''' one
        exec(compile(src, path, "exec"), ns)
    frames = sampler_frames()
    rng = np.random.default_rng(SAMPLER_SEED)
    rows = []
    for _ in range(N_DRAWS):
        ex = ns["super_batch_to_example"]({"SAT_IMAGES": _Frames(frames)}, rng=rng)
        first = ex["HISTORICAL_SAT_IMAGES"][0, 0, 0]
        hist_start, top, left = int(first // 1e6), int(first % 1e6 // 1e3), int(first % 1e3)
        assert ex["HISTORICAL_SAT_IMAGES"].shape == (4, 128, 128) and ex["TARGET_SAT_IMAGE"].shape == (64, 64)
        assert ex["TARGET_SAT_IMAGE"][0, 0] == (hist_start + 3 + int(ex["FORECAST_HORIZON"])) * 1e6 + (top + 32) * 1e3 + left + 32
        rows.append((hist_start, int(ex["FORECAST_HORIZON"]), top, left))
    out["draws"] = np.array(rows, dtype=np.int64)


def main():
    LitAutoEncoder = load_notebook_class()
    out = {}
    for tag in CASES:
        case(out, LitAutoEncoder, tag)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT) // 1024, "KiB;", len(out), "arrays")
    draws = {}
    sampler(draws)
    np.savez_compressed(OUT_SAMPLER, **draws)
    print("wrote", OUT_SAMPLER, os.path.getsize(OUT_SAMPLER), "bytes")


if __name__ == "__main__":
    main()
