"""float64 CPU restatement of notebooks/08_multiple_historical_images_as_separate_channels.ipynb's LitAutoEncoder from
torch.nn.functional, shared by tests/test_nb08_cpu.py (which pins it to the golden fixture, i.e. to the notebook's own
arithmetic) and tests/test_gpu_nb08.py (which holds the kernels to it).  The golden's inputs and initial parameters are drawn
from seeds by tests/golden/make_nb08_golden.py (draw_batch, draw_parameters)."""
import torch
import torch.nn.functional as F

from conv2d_f32_helpers import _golden_module, params64  # noqa: F401

STRIDE = (1, 2, 2)
ENCODER = (0, 2, 4)            # modules of encoder_conv: Conv3d (2, 3, 3), stride (1, 2, 2), a ReLU after each
DECODER = ((0, 2), (2, 2), (4, 1))      # (module of decoder_conv, stride): ConvTranspose2d 3x3; no ReLU after the last
G = _golden_module("nb08")


def decoder_input64(encoder_out, horizon):
    """[B, 33, e, f] float64: the encoder's output without its depth axis, then the horizon of each example as a plane."""
    out = encoder_out.squeeze(2)
    plane = torch.as_tensor(horizon).cpu().double().view(-1, 1, 1, 1).expand(out.shape[0], 1, *out.shape[2:])
    return torch.cat((out, plane), dim=1)


def _layers64(p, batch, visit=None):
    """The forward pass; visit(pre-activation z, its sum of |products|) is called for every layer a ReLU follows."""
    out = torch.as_tensor(batch["HISTORICAL_SAT_IMAGES"]).cpu().double().unsqueeze(1)
    for i in ENCODER:
        w, b = p[f"encoder_conv.{i}.weight"], p[f"encoder_conv.{i}.bias"]
        z = F.conv3d(out, w, b, stride=STRIDE)
        if visit is not None:
            visit(z, F.conv3d(out.abs(), w.abs(), b.abs(), stride=STRIDE))
        out = F.relu(z)
    out = decoder_input64(out, batch["FORECAST_HORIZON"])
    for i, stride in DECODER:
        w, b = p[f"decoder_conv.{i}.weight"], p[f"decoder_conv.{i}.bias"]
        z = F.conv_transpose2d(out, w, b, stride=stride)
        if i == DECODER[-1][0]:
            return z
        if visit is not None:
            visit(z, F.conv_transpose2d(out.abs(), w.abs(), b.abs(), stride=stride))
        out = F.relu(z)


def forward64(p, batch):
    """y_hat [B, 1, 4 e + 5, 4 f + 5]."""
    return _layers64(p, batch)


def loss64(y_hat, target):
    """F.mse_loss(y_hat[:, :, :-1, :-1], y.unsqueeze(1)) of 08_...ipynb:1396-1398."""
    target = torch.as_tensor(target).cpu().double()
    return F.mse_loss(y_hat[:, :, :-1, :-1], target.unsqueeze(1))


def relu_margin64(p, batch, tol):
    """min over every ReLU unit of |pre-activation| / (tol * its sum of |products|), in float64.  A unit below 1 lies within
    the kernels' own tolerance of 0: two correct float32 implementations may gate it differently, and one such unit moves a
    gradient by about 1 / sqrt(units) of its norm, so a fixture that holds one cannot pin gradients."""
    worst = [float("inf")]

    def visit(z, absz):
        worst[0] = min(worst[0], (z.abs() / (tol * absz)).min().item())

    with torch.no_grad():
        _layers64(p, batch, visit)
    return worst[0]


def golden_case(gold, tag):
    """(batch, initial state_dict) of golden case `tag`, redrawn from the seeds the maker used."""
    return G.draw_batch(tag), G.draw_parameters()
