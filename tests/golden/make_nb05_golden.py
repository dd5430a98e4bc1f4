"""Generates tests/golden/nb05_small.npz by EXECUTING THE REFERENCE'S OWN SOURCE on the CPU: the code cell of
notebooks/05_more_image_inputs.ipynb of the reference checkout (REF of make_conv3d_golden.py) that defines `LitAutoEncoder`
(STRIDE, GROUPS, CHANNELS and the class), exec'd as written: no statement of it is altered.
pytorch_lightning.LightningModule is the stub of make_conv3d_golden.py (torch.nn.Module + a recording log_dict).  The cell names
no device; its batch keys are the constants of an earlier cell, bound here to the strings that cell gives them.

Run where the reference checkout is (it does not travel to the GPU box):   python tests/golden/make_nb05_golden.py

Inputs and initial parameters are drawn from seeds by draw_batch / draw_parameters below (which the tests import), so the
fixture holds results only: y_hat, the three losses, the step-0 gradients and the parameters after three Adam steps of
  a/  H = W = 16, B = 3 (embedding 10 x 10), horizons of 5, 45 and 115 minutes, normalised as the loader does
  b/  H = 12, W = 20, B = 2 (embedding 6 x 14), horizons of 30 and 90 minutes; non-square
B >= 2 throughout: the notebook's x[OPTICAL_FLOW].squeeze() would drop a batch axis of size 1.
Seeds.  As make_nb10_golden.py explains, Adam's first step is lr * g / (|g| + eps), so an entry whose gradient is within
rounding of 0 moves by anything in +-lr, and a ReLU unit whose pre-activation is within rounding of 0 may be gated either way
by two correct implementations.  check_fit keeps both knives, at the notebook's lr = 1e-3 as notebook 10's maker: it runs
the same three steps in float64 (tests/nb05_reference.py) and refuses a fixture whose float32 parameters are not within
FIT_Q99 = 1e-6 of them at the 99th percentile of every tensor; and it asks, before each of the three float64 steps, that
every unit's |pre-activation| exceeds FIT_RELU_MARGIN = 3e-8 of its sum of |products|.  Each case's seed is the first from
1001 (a) / 1002 (b) up that passes both (CASES records them; main() searches again and insists on them).  Both criteria involve
the reference and float64 only, never the kernels under test.  Every tensor is stored whole (the largest has 9 504 elements).
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

OUT = os.path.join(HERE, "nb05_small.npz")
# the notebook's key constants (its "TODO: Capitalise keys" cell) and the strings it binds them to
KEYS = {"INPUT_IMAGES": "input_images", "T0_IMAGES": "T0_IMAGES", "OPTICAL_FLOW": "optical_flow",
        "FORECAST_HORIZON": "forecast_horizon", "TARGET_IMAGES": "target_images"}
CASES = {"a": dict(h=16, w=16, minutes=(5, 45, 115), seed=1001), "b": dict(h=12, w=20, minutes=(30, 90), seed=1002)}
LR = 1e-3           # the notebook's configure_optimizers
FIT_Q99 = 1e-6      # see check_fit
FIT_RELU_MARGIN = 0.03 * 1e-6      # ... of a unit's sum of |products|
FLOW_SCALE = 3.0    # pixels: the flow field is not normalised, so its planes are larger than the images'
PARAM_SHAPES = {"encoder.0.weight": (32, 4, 3, 3), "encoder.0.bias": (32,),
                "encoder.2.weight": (32, 32, 3, 3), "encoder.2.bias": (32,),
                "encoder.4.weight": (32, 32, 3, 3), "encoder.4.bias": (32,),
                "decoder.0.weight": (33, 32, 3, 3), "decoder.0.bias": (32,),
                "decoder.2.weight": (32, 32, 3, 3), "decoder.2.bias": (32,),
                "decoder.4.weight": (32, 1, 3, 3), "decoder.4.bias": (1,)}


def normalise_forecast_horizon(minutes):
    """float32 (m - 62.5) / 34.61, subtract then divide, as the notebook's super_batch_to_example does."""
    h = np.float32(minutes)
    h -= np.float32(62.5)
    h /= np.float32(34.61)
    return h


def draw_batch(tag, seed=None):
    """The case's batch: normalised-looking images (N(0, 1)), a flow field of a few pixels, the horizons as the loader's
    float32."""
    c = CASES[tag]
    g = torch.Generator().manual_seed(c["seed"] if seed is None else seed)
    b, h, w = len(c["minutes"]), c["h"], c["w"]
    return {"input_images": torch.randn(b, 1, h, w, generator=g),
            "T0_IMAGES": torch.randn(b, 1, h, w, generator=g),
            "optical_flow": torch.randn(b, 1, 2, h, w, generator=g) * FLOW_SCALE,
            "forecast_horizon": torch.tensor([normalise_forecast_horizon(m) for m in c["minutes"]], dtype=torch.float32),
            "target_images": torch.randn(b, 1, h, w, generator=g)}


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
    path = os.path.join(REF, "notebooks", "05_more_image_inputs.ipynb")
    cells = ["".join(c["source"]) for c in json.load(open(path))["cells"] if c["cell_type"] == "code"]
    (class_src,) = [c for c in cells if "class LitAutoEncoder" in c]
    (keys_src,) = [c for c in cells if c.startswith("# TODO: Capitalise keys")]
    ns = {}
    exec(compile(keys_src, path, "exec"), ns)
    assert all(ns[k] == v for k, v in KEYS.items()), "the notebook's key constants changed"
    ns.update(torch=torch, nn=nn, F=F, pl=pl)
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
    import nb05_reference as R
    batch = draw_batch(tag, seed)
    p = R.params64(draw_parameters())
    opt = torch.optim.Adam(list(p.values()), lr=LR)
    for step in range(3):
        margin = R.relu_margin64(p, batch, FIT_RELU_MARGIN)
        assert margin > 1.0, f"case {tag}: a ReLU unit within {margin:.2f} x the rounding margin of 0 at step {step}; draw another seed"
        opt.zero_grad()
        R.loss64(R.forward64(p, batch), batch["target_images"]).backward()
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
