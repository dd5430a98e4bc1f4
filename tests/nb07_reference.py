"""float64 CPU restatement of notebooks/07_multiple_historical_images.ipynb's LitAutoEncoder from torch.nn.functional, shared
by tests/test_nb07_cpu.py (which pins it to the golden fixture, i.e. to the notebook's own arithmetic) and
tests/test_gpu_nb07.py (which holds the kernels to it).  The golden's inputs and initial parameters are drawn from seeds by
tests/golden/make_nb07_golden.py (draw_batch, draw_parameters).  The encoder is applied frame by frame and the outputs are
concatenated, as the notebook does: the fold into the batch is the kernels' business and is tested against this."""
import torch
import torch.nn.functional as F

from conv2d_f32_helpers import _golden_module, params64  # noqa: F401

N_HIST_IMAGES = 4
ENCODER = (0, 2, 4)            # modules of encoder_conv: Conv2d 3x3, stride 2, a ReLU after each
DECODER = ((0, 2), (2, 2), (4, 1))      # (module of decoder_conv, stride): ConvTranspose2d 3x3; no ReLU after the last
G = _golden_module("nb07")


def frame_input64(history, horizon, f):
    """[B, 2, H, W] float64: history frame f, then the horizon of each example as a plane."""
    history = torch.as_tensor(history).cpu().double()
    plane = torch.as_tensor(horizon).cpu().double().view(-1, 1, 1, 1).expand(history.shape[0], 1, *history.shape[2:])
    return torch.cat((history[:, f:f + 1], plane), dim=1)


def folded_input64(history, horizon):
    """[F B, 2, H, W] float64 with image index F b + f: what the first layer's kernels synthesise."""
    history = torch.as_tensor(history).cpu().double()
    b, frames = history.shape[:2]
    plane = torch.as_tensor(horizon).cpu().double().view(-1, 1, 1, 1, 1).expand(b, frames, 1, *history.shape[2:])
    return torch.cat((history.unsqueeze(2), plane), dim=2).reshape(b * frames, 2, *history.shape[2:])


def _encoder64(p, x, visit):
    for i in ENCODER:
        w, b = p[f"encoder_conv.{i}.weight"], p[f"encoder_conv.{i}.bias"]
        z = F.conv2d(x, w, b, stride=2)
        if visit is not None:
            visit(z, F.conv2d(x.abs(), w.abs(), b.abs(), stride=2))
        x = F.relu(z)
    return x


def _layers64(p, batch, visit=None):
    """The forward pass; visit(pre-activation z, its sum of |products|) is called for every layer a ReLU follows."""
    frames = torch.as_tensor(batch["HISTORICAL_SAT_IMAGES"]).shape[1]
    out = torch.cat([_encoder64(p, frame_input64(batch["HISTORICAL_SAT_IMAGES"], batch["FORECAST_HORIZON"], f), visit)
                     for f in range(frames)], dim=1)
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
    """F.mse_loss(y_hat[:, :, :-1, :-1], y.unsqueeze(1)) of 07_...ipynb:1399-1402."""
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
