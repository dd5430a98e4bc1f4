"""CPU restatement of notebooks/11_just_conv_and_conv_over_time.ipynb's LitAutoEncoder from torch.nn.functional, written for
this project (the notebook hard-codes 4096 pixels and a 64 x 64 output; here P = the output's pixels), shared by
tests/test_nb11_cpu.py (which pins it to the golden fixture and to float32 torch) and tests/test_gpu_nb11.py (which holds the
kernels to it in float64).  The golden's inputs and initial parameters are drawn from seeds by
tests/golden/make_nb11_golden.py (draw_batch, draw_parameters), which runs this restatement in float32."""
import torch
import torch.nn.functional as F

from conv2d_f32_helpers import _golden_module, params64  # noqa: F401
from nb10_reference import STRIPE_WIDTH, stripe_plane64

CONVS = ((0, 0, 1), (2, 0, 1), (4, 2, 1), (6, 2, 2))       # (module of self.conv, padding, stride); a ReLU after every one
TEMPORAL = (0, 2, 4)                                       # modules of self.temporal_conv; no ReLU after the last
FRAMES = 4
G = _golden_module("nb11")


def input_frames(history, horizon, dtype=torch.float64):
    """[F B, 2, H, W]: image F b + f = (frame f of example b, the stripe plane of int(horizon[b] * 5))."""
    history = torch.as_tensor(history).cpu().to(dtype)
    b, f, h, w = history.shape
    start = (torch.as_tensor(horizon).cpu().double() * STRIPE_WIDTH).trunc()
    plane = stripe_plane64(start, h, w).to(dtype).expand(b, f, h, w)
    return torch.stack((history, plane), dim=2).reshape(b * f, 2, h, w)


def frame_stack(p, x, upto=len(CONVS)):
    """self.conv on the folded frames, through its first `upto` conv + ReLU pairs."""
    for i, pad, stride in CONVS[:upto]:
        x = F.relu(F.conv2d(x, p[f"conv.{i}.weight"], p[f"conv.{i}.bias"], stride=stride, padding=pad))
    return x


def time_image(u, frames=FRAMES):
    """[F B, 1, s1, s2] -> the notebook's [B, 1, P, F]: row p holds pixel p of the F frames' outputs."""
    fb, _, s1, s2 = u.shape
    return u.reshape(fb // frames, frames, s1 * s2).permute(0, 2, 1).unsqueeze(1)


def temporal_layers(p, t, prefix="temporal_conv."):
    """self.temporal_conv on [B, 1, P, 4] -> [B, 1, P, 1]; also returns the two hidden pre-activations."""
    z1 = F.conv2d(t, p[f"{prefix}0.weight"], p[f"{prefix}0.bias"])
    z2 = F.conv2d(F.relu(z1), p[f"{prefix}2.weight"], p[f"{prefix}2.bias"])
    return F.conv2d(F.relu(z2), p[f"{prefix}4.weight"], p[f"{prefix}4.bias"]), (z1, z2)


def forward(p, batch, dtype):
    u = frame_stack(p, input_frames(batch["HISTORICAL_SAT_IMAGES"], batch["FORECAST_HORIZON"], dtype))
    out, _ = temporal_layers(p, time_image(u))
    return out.reshape(out.shape[0], 1, *u.shape[2:])


def forward64(p, batch):
    """y_hat [B, 1, (H - 1) // 2 + 1, (W - 1) // 2 + 1] in float64 from float64 parameters."""
    return forward(p, batch, torch.float64)


def loss64(y_hat, target):
    return F.mse_loss(y_hat, torch.as_tensor(target).cpu().to(y_hat.dtype).unsqueeze(1))


def relu_margin64(p, batch, tol):
    """min over every ReLU unit (the four of self.conv, the two of self.temporal_conv) of |pre-activation| / (tol * its sum
    of |products|), in float64.  A unit below 1 lies within the kernels' own tolerance of 0: two correct float32
    implementations may gate it differently, so a fixture that holds one cannot pin gradients."""
    worst = float("inf")

    def note(z, absz):
        nonlocal worst
        worst = min(worst, (z.abs() / (tol * absz)).min().item())

    with torch.no_grad():
        out = input_frames(batch["HISTORICAL_SAT_IMAGES"], batch["FORECAST_HORIZON"])
        for i, pad, stride in CONVS:
            w, b = p[f"conv.{i}.weight"], p[f"conv.{i}.bias"]
            z = F.conv2d(out, w, b, stride=stride, padding=pad)
            note(z, F.conv2d(out.abs(), w.abs(), b.abs(), stride=stride, padding=pad))
            out = F.relu(z)
        t = time_image(out)
        for i in TEMPORAL[:-1]:
            w, b = p[f"temporal_conv.{i}.weight"], p[f"temporal_conv.{i}.bias"]
            z = F.conv2d(t, w, b)
            note(z, F.conv2d(t.abs(), w.abs(), b.abs()))
            t = F.relu(z)
    return worst
