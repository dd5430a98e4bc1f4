"""Generates tests/golden/nb15_small.npz by EXECUTING THE REFERENCE'S OWN SOURCE on the CPU: the two code cells of
/root/reference/notebooks/15_int16.ipynb that define `normalise_images_in_model` and `LitAutoEncoder` (CHANNELS, KERNEL,
STRIDE and the class), exec'd as written.  pytorch_lightning.LightningModule is the stub of make_conv3d_golden.py
(torch.nn.Module + a recording log_dict) with one attribute more: the notebook reads `self.device`, so this generator's stub
has `device = torch.device("cpu")`.  The dict-key constants are the notebook's.

Run here (the reference tree does not travel to the GPU box):   python tests/golden/make_nb15_golden.py
Two reduced cases, both from the same seeded initial state_dict (stored once):
  a/  S = 47, target 24 x 24, B = 3: sides 23, 11, 5, 2 -- every Conv2d input side is odd, every row and column is read
  b/  S = 54, target 24 x 24, B = 2: sides 26, 12, 5, 2 -- the forward leaves the last row and column of the inputs of
      layers 1, 2 and 3 unread, so their gradient is the exact zero the data-gradient kernel must write
Case b keeps its three losses but not the parameters after three steps.  History and target are int16 counts in [0, 1023],
the flow prediction float32 counts, the horizon ~ N(0, 1).  The vectors are data only.
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_conv3d_golden import REF, install_stubs  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "nb15_small.npz")
NOTEBOOK = os.path.join(REF, "notebooks", "15_int16.ipynb")
KEYS = ("FORECAST_HORIZON", "HISTORICAL_SAT_IMAGES", "OPTICAL_FLOW_PREDICTIONS", "TARGET_SAT_IMAGE")


def load_notebook_class():
    install_stubs()
    import pytorch_lightning as pl
    import torch.nn.functional as F
    from torch import nn
    pl.LightningModule.device = torch.device("cpu")
    nb = json.load(open(NOTEBOOK))
    cells = ["".join(c["source"]) for c in nb["cells"] if c["cell_type"] == "code"]
    (norm_src,) = [c for c in cells if c.lstrip().startswith("def normalise_images_in_model")]
    (class_src,) = [c for c in cells if "class LitAutoEncoder" in c]
    ns = dict(torch=torch, nn=nn, F=F, pl=pl, **{k: k for k in KEYS})
    exec(compile(norm_src, NOTEBOOK, "exec"), ns)
    exec(compile(class_src, NOTEBOOK, "exec"), ns)
    return ns["LitAutoEncoder"]


def case(out, LitAutoEncoder, tag, size, target, batch, seed, keep_step3=True):
    torch.manual_seed(42)
    model = LitAutoEncoder()
    if "init/conv.0.weight" not in out:
        for k, v in model.state_dict().items():
            out[f"init/{k}"] = v.numpy().copy()
    g = torch.Generator().manual_seed(seed)
    batch_d = {
        "HISTORICAL_SAT_IMAGES": torch.randint(0, 1024, (batch, 4, size, size), generator=g).to(torch.int16),
        "OPTICAL_FLOW_PREDICTIONS": torch.randint(0, 1024, (batch, size, size), generator=g).float()
        + torch.rand(batch, size, size, generator=g).mul(0.5),
        "FORECAST_HORIZON": torch.randn(batch, generator=g),
        "TARGET_SAT_IMAGE": torch.randint(0, 1024, (batch, target, target), generator=g).to(torch.int16)}
    for k, v in batch_d.items():
        out[f"{tag}/{k}"] = v.numpy()
    out[f"{tag}/y_hat"] = model(batch_d).detach().numpy().copy()
    opt = model.configure_optimizers()
    losses = []
    for step in range(3):
        opt.zero_grad()
        loss = model.training_step(batch_d, 0)
        loss.backward()
        if step == 0:
            for k, p in model.named_parameters():
                out[f"{tag}/grad/{k}"] = p.grad.numpy().copy()
        opt.step()
        losses.append(float(loss.detach()))
    if keep_step3:
        for k, p in model.named_parameters():
            out[f"{tag}/step3/{k}"] = p.detach().numpy().copy()
    out[f"{tag}/losses"] = np.array(losses)


def main():
    LitAutoEncoder = load_notebook_class()
    out = {}
    case(out, LitAutoEncoder, "a", size=47, target=24, batch=3, seed=1501)
    case(out, LitAutoEncoder, "b", size=54, target=24, batch=2, seed=1502, keep_step3=False)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT) // 1024, "KiB;", len(out), "arrays")


if __name__ == "__main__":
    main()
