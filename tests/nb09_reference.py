"""float64 CPU restatement of notebooks/09_horizon_represented_as_a_stripe.ipynb's LitAutoEncoder from torch.nn.functional,
shared by tests/test_nb09_cpu.py (which pins it to the golden fixture, i.e. to the notebook's own arithmetic) and
tests/test_gpu_nb09.py (which holds the kernels to it).  The golden's inputs and initial parameters are drawn from seeds by
tests/golden/make_nb09_golden.py (draw_batch, draw_parameters), which also names the stored entries of a sampled tensor.
The stripe plane, the stored-entry checks and the parameter conversion are notebook 10's (tests/nb10_reference.py)."""
import torch
import torch.nn.functional as F

from conv2d_f32_helpers import _golden_module
from nb10_reference import STRIPE_WIDTH, input64, params64, stripe_plane64  # noqa: F401

ENCODER = (0, 2, 4)        # modules of encoder_conv: Conv2d, stride 2, a ReLU after each
DECODER = ((0, 2), (2, 2), (4, 1))      # (module of decoder_conv, stride): ConvTranspose2d; no ReLU after the last
G = _golden_module("nb09")


def _layers(p):
    """(function, weight, bias, stride, relu) of the six layers in order."""
    out = [(F.conv2d, p[f"encoder_conv.{i}.weight"], p[f"encoder_conv.{i}.bias"], 2, True) for i in ENCODER]
    out += [(F.conv_transpose2d, p[f"decoder_conv.{i}.weight"], p[f"decoder_conv.{i}.bias"], s, i != DECODER[-1][0])
            for i, s in DECODER]
    return out


def forward64(p, batch):
    """y_hat [B, 1, 4 e(H) + 5, 4 e(W) + 5], e = three times s -> (s - 3) // 2 + 1."""
    out = input64(batch["HISTORICAL_SAT_IMAGES"], batch["FORECAST_HORIZON"])
    for fn, w, b, stride, relu in _layers(p):
        out = fn(out, w, b, stride=stride)
        if relu:
            out = F.relu(out)
    return out


def loss64(y_hat, target):
    return F.mse_loss(y_hat[:, :, :-1, :-1], torch.as_tensor(target).cpu().double().unsqueeze(1))


def stored(name, t):
    """The entries of tensor t the golden stores under `name`, with the tensor's float64 (sum, norm) where it is sampled."""
    t = torch.as_tensor(t).detach().cpu().double()
    idx = G.sample_index(name, t.numel())
    if idx is None:
        return t, None
    return t.flatten()[torch.from_numpy(idx)], (t.sum().item(), t.norm().item())


def check_stored(gold, name, t, tol, entries_only=False):
    """t against the golden entry `name` to relative norm tol: the stored entries, and for a sampled tensor also its norm
    (to tol) and its sum (|sum(a) - sum(b)| <= sqrt(numel) |a - b| <= sqrt(numel) tol |b|).  Returns the entries' error."""
    got, stats = stored(name, t)
    want = torch.from_numpy(gold[name]).double().reshape(got.shape)
    err = ((got - want).norm() / (want.norm() + 1e-30)).item()
    if entries_only:
        return err
    assert err <= tol, (name, err)
    if stats is not None:
        gsum, gnorm = float(gold[name + "/sum"]), float(gold[name + "/norm"])
        assert abs(stats[1] - gnorm) <= tol * gnorm, (name, stats[1], gnorm)
        assert abs(stats[0] - gsum) <= torch.as_tensor(t).numel() ** 0.5 * tol * gnorm, (name, stats[0], gsum)
    return err


def relu_margin64(p, batch, tol):
    """min over every ReLU unit (encoder and decoder) of |pre-activation| / (tol * its sum of |products|), in float64.  A
    unit below 1 lies within the kernels' own tolerance of 0: two correct float32 implementations may gate it differently,
    and one such unit moves a gradient by about 1 / sqrt(units) of its norm, so a fixture that holds one cannot pin
    gradients."""
    out = input64(batch["HISTORICAL_SAT_IMAGES"], batch["FORECAST_HORIZON"])
    worst = float("inf")
    with torch.no_grad():
        for fn, w, b, stride, relu in _layers(p):
            if not relu:
                break
            z = fn(out, w, b, stride=stride)
            absz = fn(out.abs(), w.abs(), b.abs(), stride=stride)
            worst = min(worst, (z.abs() / (tol * absz)).min().item())
            out = F.relu(z)
    return worst
