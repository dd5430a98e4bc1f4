"""Generates tests/golden/nb09_small.npz by EXECUTING THE REFERENCE'S OWN SOURCE on the CPU: the code cell of
notebooks/09_horizon_represented_as_a_stripe.ipynb of the reference checkout (REF of make_conv3d_golden.py) that defines
`LitAutoEncoder` (STRIDE, CHANNELS, N_HIST_IMAGES, STRIPE_WIDTH and the class), exec'd as written, exactly as
make_nb10_golden.py does for notebook 10: pytorch_lightning.LightningModule is the stub of make_conv3d_golden.py, and the
`torch` name the cell sees forwards everything to torch except that `zeros` drops the device argument, so the stripe plane
lands on the CPU.  Nothing else of the cell is altered.

Run where the reference checkout is:   python tests/golden/make_nb09_golden.py

Inputs and initial parameters are drawn from seeds by draw_batch / draw_parameters below (which the tests import), so the
fixture holds results only: y_hat, the three losses, the step-0 gradients and the parameters after three Adam steps of
  a/  H = W = 47, B = 3, horizons 1, 9, 23: a stripe inside the image, one clipped at the right edge and an empty one; odd
      sides throughout (47 -> 23 -> 11 -> 5, output 25)
  b/  H = 20, W = 54, B = 2, horizons 0, 10: the stripe at column 0 and one clipped at the edge; even sides with an unread
      last row / column at every encoder layer and a one-row bottleneck (20 -> 9 -> 4 -> 1; 54 -> 26 -> 12 -> 5; output 9 x 25)
Seeds.  check_fit keeps both conditions of make_nb10_golden.py (see there for why): the notebook model's float32 parameters
after three steps lie within FIT_Q99 = 1e-6 of the same steps in float64 (tests/nb09_reference.py) at the 99th percentile of
every tensor, and before each float64 step every ReLU unit's |pre-activation| (encoder and decoder) exceeds FIT_RELU_MARGIN
= 3e-8 of its sum of |products|.  Each case's seed is the first from 1001 (a) / 1002 (b) up that passes both.  Both criteria
involve the reference and float64 only, never the kernels under test.
A tensor above 20 000 elements is stored as 4 096 seeded entries (sample_index) plus its float64 sum and norm.
The generator also asserts that notebook 09's sampler cells (sample_squares, super_batch_to_example, normalise_images,
SatelliteLoader) equal notebook 10's character for character: that is why Nb10DataModule serves this model unchanged.
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_nb10_golden import KEYS, sample_index, store  # noqa: E402,F401  (one storage rule for both notebooks)

OUT = os.path.join(HERE, "nb09_small.npz")
NOTEBOOK = "09_horizon_represented_as_a_stripe.ipynb"
CASES = {"a": dict(h=47, w=47, horizons=(1, 9, 23), seed=1001), "b": dict(h=20, w=54, horizons=(0, 10), seed=1002)}
FIT_Q99 = 1e-6      # see check_fit
FIT_RELU_MARGIN = 0.03 * 1e-6      # ... of a unit's sum of |products|
PARAM_SHAPES = {"encoder_conv.0.weight": (64, 5, 3, 3), "encoder_conv.0.bias": (64,),
                "encoder_conv.2.weight": (128, 64, 3, 3), "encoder_conv.2.bias": (128,),
                "encoder_conv.4.weight": (128, 128, 3, 3), "encoder_conv.4.bias": (128,),
                "decoder_conv.0.weight": (128, 128, 3, 3), "decoder_conv.0.bias": (128,),
                "decoder_conv.2.weight": (128, 128, 3, 3), "decoder_conv.2.bias": (128,),
                "decoder_conv.4.weight": (128, 1, 3, 3), "decoder_conv.4.bias": (1,)}
SAMPLER_CELLS = ("def sample_squares", "def super_batch_to_example", "def normalise_images", "TIMESTEPS_PER_HOUR = 12")


def out_side(s):
    for _ in range(3):
        s = (s - 3) // 2 + 1
    return 4 * s + 5


def draw_batch(tag):
    """The case's batch: normalised-looking history and target (N(0, 1)), the horizons as int64; the target is one smaller
    than the output on each side (the loss drops the prediction's last row and column)."""
    c = CASES[tag]
    g = torch.Generator().manual_seed(c["seed"])
    b = len(c["horizons"])
    return {"HISTORICAL_SAT_IMAGES": torch.randn(b, 4, c["h"], c["w"], generator=g),
            "FORECAST_HORIZON": torch.tensor(c["horizons"], dtype=torch.int64),
            "TARGET_SAT_IMAGE": torch.randn(b, out_side(c["h"]) - 1, out_side(c["w"]) - 1, generator=g)}


def fan_in(key):
    """Of the layer that owns parameter `key`, as nn.Conv2d / nn.ConvTranspose2d count it: weight.size(1) * 9."""
    return PARAM_SHAPES[key.replace("bias", "weight")][1] * 9


def draw_parameters(seed=1000):
    """The initial state_dict: uniform in +-1 / sqrt(fan_in), the range of torch's own initialisation."""
    g = torch.Generator().manual_seed(seed)
    return {k: (torch.rand(*shape, generator=g) * 2 - 1) * fan_in(k) ** -0.5 for k, shape in PARAM_SHAPES.items()}


def _notebook_cells(name):
    from make_conv3d_golden import REF
    path = os.path.join(REF, "notebooks", name)
    nb = json.load(open(path))
    return path, ["".join(c["source"]) for c in nb["cells"] if c["cell_type"] == "code"]


def check_sampler_cells_equal_notebook_10():
    _, mine = _notebook_cells(NOTEBOOK)
    _, theirs = _notebook_cells("10_just_conv.ipynb")
    for marker in SAMPLER_CELLS:
        a = [c for c in mine if c.lstrip().startswith(marker)]
        b = [c for c in theirs if c.lstrip().startswith(marker)]
        assert a and a[-1] == b[-1], f"notebook 09's cell '{marker}' differs from notebook 10's"


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

    path, cells = _notebook_cells(NOTEBOOK)
    (class_src,) = [c for c in cells if "class LitAutoEncoder" in c]
    ns = dict(torch=_TorchOnCpu("torch"), nn=nn, F=F, pl=pl, **{k: k for k in KEYS})
    exec(compile(class_src, path, "exec"), ns)
    return ns["LitAutoEncoder"]


def case(out, LitAutoEncoder, tag):
    model = LitAutoEncoder()
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == PARAM_SHAPES
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
    import nb09_reference as R
    batch = draw_batch(tag)
    p = R.params64(draw_parameters())
    opt = torch.optim.Adam(list(p.values()), lr=0.001)
    worst = float("inf")
    for step in range(3):
        margin = R.relu_margin64(p, batch, FIT_RELU_MARGIN)
        worst = min(worst, margin)
        assert margin > 1.0, f"case {tag}: a ReLU unit within {margin:.2f} x the rounding margin of 0 at step {step}; draw another seed"
        opt.zero_grad()
        R.loss64(R.forward64(p, batch), batch["TARGET_SAT_IMAGE"]).backward()
        opt.step()
    q99s, moved = [], []
    init = draw_parameters()
    for k, v in model.named_parameters():
        err = (v.detach().double() - p[k].detach()).abs().flatten().sort().values
        q99 = err[int(0.99 * (err.numel() - 1))].item()
        assert q99 <= FIT_Q99, f"case {tag}: {k} differs from float64 by {q99:.2e} at the 99th percentile; draw another seed"
        q99s.append(q99)
        moved.append((v.detach() - init[k]).abs().median().item())
    print(f"case {tag} seed {CASES[tag]['seed']}: ReLU margin {worst:.1f} x, q99 {max(q99s):.1e}, smallest median parameter "
          f"movement {min(moved):.1e}")


def main():
    check_sampler_cells_equal_notebook_10()
    LitAutoEncoder = load_notebook_class()
    out = {}
    for tag in CASES:
        case(out, LitAutoEncoder, tag)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT) // 1024, "KiB;", len(out), "arrays")


if __name__ == "__main__":
    main()
