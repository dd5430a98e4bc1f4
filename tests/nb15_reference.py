"""float64 CPU restatement of notebooks/15_int16.ipynb's LitAutoEncoder from torch.nn.functional, shared by
tests/test_nb15_cpu.py (which pins it to the golden fixture, i.e. to the notebook's own arithmetic) and tests/test_gpu_nb15.py
(which holds the kernels to it)."""
import numpy as np
import torch
import torch.nn.functional as F

from conv2d_f32_helpers import params64  # noqa: F401

MEAN = float(np.float32(93.23458))
STD = float(np.float32(115.34247))
ENC = (0, 2, 4, 6)       # nn.Conv2d modules of self.conv, stride 2
DEC = (8, 10, 12)        # nn.ConvTranspose2d modules, stride 2; no ReLU after the last


def normalise64(counts):
    return (torch.as_tensor(counts).double() - MEAN) / STD


def input64(history, flow_pred, horizon):
    """[B, 6, S, S] float64: normalised history and flow prediction, then the horizon plane (not normalised again)."""
    history, flow_pred, horizon = (torch.as_tensor(t).cpu() for t in (history, flow_pred, horizon))
    images = normalise64(torch.cat((history.double(), flow_pred.double().unsqueeze(1)), dim=1))
    b, _, h, w = images.shape
    return torch.cat((images, horizon.double().view(-1, 1, 1, 1).expand(b, 1, h, w)), dim=1)


def forward64(p, batch):
    """y_hat [B, 1, P, P]."""
    out = input64(batch["HISTORICAL_SAT_IMAGES"], batch["OPTICAL_FLOW_PREDICTIONS"], batch["FORECAST_HORIZON"])
    for i in ENC:
        out = F.relu(F.conv2d(out, p[f"conv.{i}.weight"], p[f"conv.{i}.bias"], stride=2))
    for i in DEC:
        out = F.conv_transpose2d(out, p[f"conv.{i}.weight"], p[f"conv.{i}.bias"], stride=2)
        if i != DEC[-1]:
            out = F.relu(out)
    return out


def loss64(y_hat, target):
    y = normalise64(torch.as_tensor(target).cpu())[..., :-1, :-1]
    assert tuple(y.shape) == tuple(y_hat.squeeze(1).shape), (y.shape, y_hat.shape)
    return F.mse_loss(y_hat.squeeze(1), y)


def golden_case(gold, tag):
    keys = ("HISTORICAL_SAT_IMAGES", "OPTICAL_FLOW_PREDICTIONS", "FORECAST_HORIZON", "TARGET_SAT_IMAGE")
    batch = {k: torch.from_numpy(gold[f"{tag}/{k}"]) for k in keys}
    init = {k[len("init/"):]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("init/")}
    return batch, init
