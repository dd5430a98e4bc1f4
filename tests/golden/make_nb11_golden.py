"""Generates tests/golden/nb11_small.npz on the CPU from the project's own restatement of
notebooks/11_just_conv_and_conv_over_time.ipynb's LitAutoEncoder (tests/nb11_reference.py) run in float32 with torch's own
Adam(lr=1e-4), the notebook's optimiser.  The notebook's class cell cannot be run at these sizes: its forward hard-codes 4096
pixels per frame and a 64 x 64 output, i.e. 128 x 128 inputs only, which is too large for a fixture; the restatement takes P
from the input's sides and is otherwise the cell's arithmetic (tests/test_nb11_cpu.py holds it to a float32 nn.Module built
from the model file's layers).

Run from the repository root:   python tests/golden/make_nb11_golden.py

Inputs and initial parameters are drawn from seeds by draw_batch / draw_parameters below (which the tests import), so the
fixture holds results only: y_hat, the three losses, the step-0 gradients and the parameters after three Adam steps of
  a/  H = W = 12, B = 2, horizons 1, 2: a stripe inside the image (columns 5..9) and one clipped at the right edge (columns
      10, 11 of 10..14); y_hat 6 x 6
  b/  H = W = 21, B = 2, horizons 0, 23: the stripe at column 0 and an empty one (start 115 >= W); y_hat 11 x 11
Seeds, as for notebook 10's fixture (make_nb10_golden.py has the reasoning): an entry whose gradient is within rounding of 0, or a
ReLU unit whose pre-activation is, may go either way in two correct implementations, and then the parameters after three steps
cannot be pinned.  check_fit runs the same three steps in float64 and refuses a fixture whose float32 parameters are not within
FIT_Q99 of them at the 99th percentile of every tensor (a tenth of what the tests ask of the kernels at this learning rate),
or in which, before any of the three float64 steps, a unit's |pre-activation| is below FIT_RELU_MARGIN = 3e-8 of its sum of
|products|.  Each case's seed is the first from 1101 (a) / 1102 (b) up that passes both (a: 1102 -- 1101 puts a unit at 0.27 of the
margin before the second step --, b: 1102); main() searches when a recorded seed
no longer does.  Both criteria involve this restatement in float32 and float64 only, never the kernels under test.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

OUT = os.path.join(HERE, "nb11_small.npz")
CASES = {"a": dict(h=12, w=12, horizons=(1, 2), seed=1102), "b": dict(h=21, w=21, horizons=(0, 23), seed=1102)}
LR = 1e-4
FIT_Q99 = 1e-7      # see check_fit
FIT_RELU_MARGIN = 0.03 * 1e-6      # ... of a unit's sum of |products|
PARAM_SHAPES = {"conv.0.weight": (16, 2, 3, 3), "conv.0.bias": (16,), "conv.2.weight": (32, 16, 3, 3), "conv.2.bias": (32,),
                "conv.4.weight": (32, 32, 3, 3), "conv.4.bias": (32,), "conv.6.weight": (1, 32, 3, 3), "conv.6.bias": (1,),
                "temporal_conv.0.weight": (16, 1, 1, 2), "temporal_conv.0.bias": (16,),
                "temporal_conv.2.weight": (16, 16, 1, 2), "temporal_conv.2.bias": (16,),
                "temporal_conv.4.weight": (1, 16, 1, 2), "temporal_conv.4.bias": (1,)}


def out_side(s):
    return (s - 1) // 2 + 1


def draw_batch(tag, seed=None):
    """The case's batch: normalised-looking history and target (N(0, 1)), the horizons as int64."""
    c = CASES[tag]
    g = torch.Generator().manual_seed(c["seed"] if seed is None else seed)
    b = len(c["horizons"])
    return {"HISTORICAL_SAT_IMAGES": torch.randn(b, 4, c["h"], c["w"], generator=g),
            "FORECAST_HORIZON": torch.tensor(c["horizons"], dtype=torch.int64),
            "TARGET_SAT_IMAGE": torch.randn(b, out_side(c["h"]), out_side(c["w"]), generator=g)}


def draw_parameters(seed=1100):
    """The initial state_dict: uniform in +-1 / sqrt(fan_in), the range of nn.Conv2d's own initialisation, except that the two
    hidden biases of temporal_conv are made non-negative.  That network's inputs are the head's ReLU outputs, small and >= 0,
    so a hidden unit's sign is its bias's: with signed biases half the units are dead for every pixel, three quarters of
    temporal_conv.2.weight has an exactly zero gradient, and the parameters after three steps would pin nothing there."""
    g = torch.Generator().manual_seed(seed)
    state = {}
    for k, shape in PARAM_SHAPES.items():
        fan_in = int(np.prod(PARAM_SHAPES[k.replace("bias", "weight")][1:]))
        state[k] = (torch.rand(*shape, generator=g) * 2 - 1) * fan_in ** -0.5
        if k in ("temporal_conv.0.bias", "temporal_conv.2.bias"):
            state[k] = state[k].abs()
    return state


def _reference():
    sys.path.insert(0, os.path.dirname(HERE))
    import nb11_reference as R
    return R


def _three_steps(R, batch, dtype, before_step=None):
    """Three Adam steps of the restatement in `dtype`: (parameters, y_hat before the first step, step-0 gradients, losses)."""
    p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in draw_parameters().items()}
    opt = torch.optim.Adam(list(p.values()), lr=LR)
    y_hat, grads, losses = None, None, []
    for step in range(3):
        if before_step is not None:
            before_step(step, p)
        opt.zero_grad()
        y = R.forward(p, batch, dtype)
        loss = R.loss64(y, batch["TARGET_SAT_IMAGE"])
        loss.backward()
        if step == 0:
            y_hat, grads = y.detach().clone(), {k: v.grad.detach().clone() for k, v in p.items()}
        opt.step()
        losses.append(float(loss.detach()))
    return p, y_hat, grads, losses


def check_fit(tag, p32):
    """The float32 parameters after three steps against the same steps in float64; every ReLU unit clear of 0 before each."""
    R = _reference()
    batch = draw_batch(tag)

    def margin(step, p):
        m = R.relu_margin64(p, batch, FIT_RELU_MARGIN)
        assert m > 1.0, f"case {tag}: a ReLU unit within {m:.2f} x the rounding margin of 0 at step {step}; draw another seed"

    p64, *_ = _three_steps(R, batch, torch.float64, before_step=margin)
    for k, v in p32.items():
        err = (v.detach().double() - p64[k].detach()).abs().flatten().sort().values
        q99 = err[int(0.99 * (err.numel() - 1))].item()
        assert q99 <= FIT_Q99, f"case {tag}: {k} differs from float64 by {q99:.2e} at the 99th percentile; draw another seed"


def case(out, tag):
    R = _reference()
    p, y_hat, grads, losses = _three_steps(R, draw_batch(tag), torch.float32)
    check_fit(tag, p)
    out[f"{tag}/y_hat"] = y_hat.numpy().copy()
    for k in p:
        out[f"{tag}/grad/{k}"] = grads[k].numpy().copy()
        out[f"{tag}/step3/{k}"] = p[k].detach().numpy().copy()
    out[f"{tag}/losses"] = np.array(losses)


def main():
    out = {}
    for tag in CASES:
        first = CASES[tag]["seed"]
        for seed in range(first, first + 50):
            CASES[tag]["seed"] = seed
            try:
                case(out, tag)
                break
            except AssertionError as e:
                print(e)
        else:
            raise SystemExit(f"case {tag}: no seed in {first}..{first + 49} passes check_fit")
        print(f"case {tag}: seed {seed}" + ("" if seed == first else f" -- record it in CASES (was {first})"))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT) // 1024, "KiB;", len(out), "arrays")


if __name__ == "__main__":
    main()
