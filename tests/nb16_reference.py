"""float64 CPU restatement of notebooks/16_maxpool.ipynb's LitAutoEncoder from torch.nn.functional, shared by
tests/test_nb16_cpu.py (which pins it to the golden fixture, i.e. to the notebook's own arithmetic) and tests/test_gpu_nb16.py
(which holds the kernels to it)."""
import numpy as np
import torch
import torch.nn.functional as F

from conv2d_f32_helpers import params64  # noqa: F401

MEAN = float(np.float32(93.23458))
STD = float(np.float32(115.34247))
ENC = ("encoder_conv1", "encoder_conv2", "encoder_conv3", "encoder_conv4")
DEC = ("decoder_conv1", "decoder_conv2", "decoder_conv3", "decoder_conv4")
ROUTED_TOL = 2e-2    # gradients below the pool against another implementation's window picks (tests/test_gpu_exp001.py)


def normalise64(counts):
    return (torch.as_tensor(counts).double() - MEAN) / STD


def input64(history, flow_pred, horizon):
    """[B, 6, S, S] float64: normalised history and flow prediction, then the horizon plane (not normalised again)."""
    history, flow_pred, horizon = (torch.as_tensor(t).cpu() for t in (history, flow_pred, horizon))
    images = normalise64(torch.cat((history.double(), flow_pred.double().unsqueeze(1)), dim=1))
    b, _, h, w = images.shape
    return torch.cat((images, horizon.double().view(-1, 1, 1, 1).expand(b, 1, h, w)), dim=1)


def encoder_pre64(p, x):
    """Pre-activation of encoder_conv4 (the tensor the pool looks at) in float64."""
    out = x
    for name in ENC[:3]:
        out = F.relu(F.conv2d(out, p[f"{name}.weight"], p[f"{name}.bias"]))
    return F.conv2d(out, p["encoder_conv4.weight"], p["encoder_conv4.bias"])


def decoder64(p, pooled):
    out = pooled
    for name in DEC[:3]:
        out = F.relu(F.conv_transpose2d(out, p[f"{name}.weight"], p[f"{name}.bias"]))
    return F.conv_transpose2d(out, p["decoder_conv4.weight"], p["decoder_conv4.bias"])


def forward64(p, batch, pool=None):
    """y_hat [B, 1, P + 8, P + 8]; pool(z) -> pooled replaces max_pool2d(relu(z), 3) (e.g. routing through given codes)."""
    x = input64(batch["HISTORICAL_SAT_IMAGES"], batch["OPTICAL_FLOW_PREDICTIONS"], batch["FORECAST_HORIZON"])
    z = encoder_pre64(p, x)
    pooled = pool(z) if pool is not None else F.max_pool2d(F.relu(z), 3)
    return decoder64(p, pooled)


def loss64(y_hat, target):
    y = normalise64(torch.as_tensor(target).cpu())[..., 8:-8, 8:-8]
    assert tuple(y.shape) == tuple(y_hat.squeeze(1).shape), (y.shape, y_hat.shape)
    return F.mse_loss(y_hat.squeeze(1), y)


def golden_case(gold, tag):
    keys = ("HISTORICAL_SAT_IMAGES", "OPTICAL_FLOW_PREDICTIONS", "FORECAST_HORIZON", "TARGET_SAT_IMAGE")
    batch = {k: torch.from_numpy(gold[f"{tag}/{k}"]) for k in keys}
    init = {k[len("init/"):]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("init/")}
    return batch, init
