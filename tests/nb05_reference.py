"""float64 CPU restatement of notebooks/05_more_image_inputs.ipynb's LitAutoEncoder from torch.nn.functional, shared by
tests/test_nb05_cpu.py (which pins it to the golden fixture, i.e. to the notebook's own arithmetic) and tests/test_gpu_nb05.py
(which holds the kernels to it).  The golden's inputs and initial parameters are drawn from seeds by
tests/golden/make_nb05_golden.py (draw_batch, draw_parameters)."""
import torch
import torch.nn.functional as F

from conv2d_f32_helpers import _golden_module, params64  # noqa: F401

ENCODER = (0, 2, 4)            # modules of encoder: Conv2d 3x3, a ReLU after each
DECODER = (0, 2, 4)            # modules of decoder: ConvTranspose2d 3x3; no ReLU after the last
G = _golden_module("nb05")


def encoder_input64(batch):
    """[B, 4, H, W] float64: the flow prediction, the t0 image, then the x and y planes of the flow field.  The field's
    singleton axis is dropped by shape, so the batch axis survives B = 1."""
    pred = torch.as_tensor(batch["input_images"]).cpu().double()
    t0 = torch.as_tensor(batch["T0_IMAGES"]).cpu().double()
    field = torch.as_tensor(batch["optical_flow"]).cpu().double()
    return torch.cat((pred, t0, field.reshape(pred.shape[0], 2, *pred.shape[2:])), dim=1)


def decoder_input64(embedding, horizon):
    """[B, 33, e, f] float64: the embedding, then the horizon of each example as a plane."""
    plane = torch.as_tensor(horizon).cpu().double().view(-1, 1, 1, 1).expand(embedding.shape[0], 1, *embedding.shape[2:])
    return torch.cat((embedding, plane), dim=1)


def _layers64(p, batch, visit=None):
    """The forward pass; visit(pre-activation z, its sum of |products|) is called for every layer a ReLU follows."""
    out = encoder_input64(batch)
    for i in ENCODER:
        w, b = p[f"encoder.{i}.weight"], p[f"encoder.{i}.bias"]
        z = F.conv2d(out, w, b)
        if visit is not None:
            visit(z, F.conv2d(out.abs(), w.abs(), b.abs()))
        out = F.relu(z)
    out = decoder_input64(out, batch["forecast_horizon"])
    for i in DECODER:
        w, b = p[f"decoder.{i}.weight"], p[f"decoder.{i}.bias"]
        z = F.conv_transpose2d(out, w, b)
        if i == DECODER[-1]:
            return z
        if visit is not None:
            visit(z, F.conv_transpose2d(out.abs(), w.abs(), b.abs()))
        out = F.relu(z)


def forward64(p, batch):
    """y_hat [B, 1, H, W]."""
    return _layers64(p, batch)


def loss64(y_hat, target):
    """F.mse_loss(y_hat, y) of 05_more_image_inputs.ipynb:1394, both [B, 1, H, W]."""
    return F.mse_loss(y_hat, torch.as_tensor(target).cpu().double())


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
