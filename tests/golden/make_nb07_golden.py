"""Generates tests/golden/nb07_small.npz by EXECUTING THE REFERENCE'S OWN SOURCE on the CPU: the code cell of
notebooks/07_multiple_historical_images.ipynb of the reference checkout (REF of make_conv3d_golden.py) that defines
`LitAutoEncoder` (STRIDE, CHANNELS, N_HIST_IMAGES and the class), exec'd as written, without alteration: nothing in it is in
place.  pytorch_lightning.LightningModule is the stub of make_conv3d_golden.py (torch.nn.Module + a recording log_dict).  The
cell names no device.

Run where the reference checkout is (it does not travel to the GPU box):   python tests/golden/make_nb07_golden.py

Inputs and initial parameters are drawn from seeds by draw_batch / draw_parameters below (which the tests import), so the
fixture holds results only: y_hat, the three losses, the step-0 gradients and the parameters after three Adam steps of
  a/  H = W = 31, B = 3 (output 17 x 17, target 16 x 16), horizons of 1, 9 and 23 timesteps, normalised as the loader does
  b/  H = 23, W = 39, B = 2 (output 13 x 21, target 12 x 20), horizons of 12 and 24 timesteps; non-square
Seeds.  As make_nb10_golden.py explains, Adam's first step is lr * g / (|g| + eps), so an entry whose gradient is within
rounding of 0 moves by anything in +-lr, and a ReLU unit whose pre-activation is within rounding of 0 may be gated either way
by two correct implementations.  check_fit keeps both knives, at the notebook's lr = 1e-3 as notebook 08's maker: it runs
the same three steps in float64 (tests/nb07_reference.py) and refuses a fixture whose float32 parameters are not within
FIT_Q99 = 1e-6 of them at the 99th percentile of every tensor; and it asks, before each of the three float64 steps, that
every unit's |pre-activation| exceeds FIT_RELU_MARGIN = 3e-8 of its sum of |products|.  Each case's seed is the first from
1001 (a) / 1002 (b) up that passes both (a: 1002, since 1001 leaves encoder_conv.0.weight 2.3e-5 from float64 at the 99th
percentile; b: 1002 at its first draw; CASES records them, main() searches again and insists on them).  Both criteria
involve the reference and float64 only, never the kernels under test.  Every tensor is stored whole (the largest has 36 864
elements).
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

OUT = os.path.join(HERE, "nb07_small.npz")
KEYS = ("FORECAST_HORIZON", "HISTORICAL_SAT_IMAGES", "TARGET_SAT_IMAGE")
CASES = {"a": dict(h=31, w=31, timesteps=(1, 9, 23), seed=1002), "b": dict(h=23, w=39, timesteps=(12, 24), seed=1002)}
LR = 1e-3           # the notebook's configure_optimizers
FIT_Q99 = 1e-6      # see check_fit
FIT_RELU_MARGIN = 0.03 * 1e-6      # ... of a unit's sum of |products|
PARAM_SHAPES = {"encoder_conv.0.weight": (32, 2, 3, 3), "encoder_conv.0.bias": (32,),
                "encoder_conv.2.weight": (32, 32, 3, 3), "encoder_conv.2.bias": (32,),
                "encoder_conv.4.weight": (32, 32, 3, 3), "encoder_conv.4.bias": (32,),
                "decoder_conv.0.weight": (128, 32, 3, 3), "decoder_conv.0.bias": (32,),
                "decoder_conv.2.weight": (32, 32, 3, 3), "decoder_conv.2.bias": (32,),
                "decoder_conv.4.weight": (32, 1, 3, 3), "decoder_conv.4.bias": (1,)}


def out_side(s):
    for _ in range(3):
        s = (s - 3) // 2 + 1
    return 4 * s + 5


def normalise_forecast_horizon(timesteps):
    """float32 (h - mean) / std of arange(1, 25), as the loaders of notebooks 07, 08 and 12 do."""
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
            "TARGET_SAT_IMAGE": torch.randn(b, out_side(c["h"]) - 1, out_side(c["w"]) - 1, generator=g)}


def draw_parameters(seed=1000):
    """The initial state_dict: uniform in +-1 / sqrt(fan_in) of the weight's trailing axes, the scale of torch's own
    initialisation."""
    g = torch.Generator().manual_seed(seed)
    state = {}
    for k, shape in PARAM_SHAPES.items():
        fan_in = int(np.prod(PARAM_SHAPES[k.replace("bias", "weight")][1:]))
        state[k] = (torch.rand(*shape, generator=g) * 2 - 1) * fan_in ** -0.5
    return state


def load_notebook_class():
    from make_conv3d_golden import REF, install_stubs
    install_stubs()
    import pytorch_lightning as pl
    import torch.nn.functional as F
    from torch import nn
    path = os.path.join(REF, "notebooks", "07_multiple_historical_images.ipynb")
    cells = ["".join(c["source"]) for c in json.load(open(path))["cells"] if c["cell_type"] == "code"]
    (class_src,) = [c for c in cells if "class LitAutoEncoder" in c]
    ns = dict(torch=torch, nn=nn, F=F, pl=pl, **{k: k for k in KEYS})
    exec(compile(class_src, path, "exec"), ns)
    return ns["LitAutoEncoder"]


def case(out, LitAutoEncoder, tag, seed=None):
    model = LitAutoEncoder()
    model.load_state_dict(draw_parameters())
    batch = draw_batch(tag, seed)
    out[f"{tag}/y_hat"] = model(batch).detach().numpy().copy()
    opt = model.configure_optimizers()
    assert opt.param_groups[0]["lr"] == LR
    losses = []
    for step in range(3):
        opt.zero_grad()
        loss = model.training_step(batch, 0)
        loss.backward()
        if step == 0:
            for k, p in model.named_parameters():
                out[f"{tag}/grad/{k}"] = p.grad.detach().numpy().copy()
        opt.step()
        losses.append(float(loss.detach()))
    for k, p in model.named_parameters():
        out[f"{tag}/step3/{k}"] = p.detach().numpy().copy()
    out[f"{tag}/losses"] = np.array(losses)
    check_fit(tag, model, seed)


def check_fit(tag, model, seed=None):
    """The notebook model's float32 parameters after its three steps against the same steps in float64."""
    sys.path.insert(0, os.path.dirname(HERE))
    import nb07_reference as R
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
    for tag, first in (("a", 1001), ("b", 1002)):
        for seed in range(first, first + 64):       # the first seed that passes check_fit; CASES must record it
            trial = {}
            try:
                case(trial, LitAutoEncoder, tag, seed)
            except AssertionError as e:
                print(f"case {tag} seed {seed}: {e}")
                continue
            assert seed == CASES[tag]["seed"], f"case {tag}: the first passing seed is {seed}; record it in CASES"
            out.update(trial)
            break
        else:
            raise SystemExit(f"case {tag}: no seed passed")
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT) // 1024, "KiB;", len(out), "arrays")


if __name__ == "__main__":
    main()
