"""float64 CPU restatement of notebooks/10_just_conv.ipynb's LitAutoEncoder from torch.nn.functional, shared by
tests/test_nb10_cpu.py (which pins it to the golden fixture, i.e. to the notebook's own arithmetic) and tests/test_gpu_nb10.py
(which holds the kernels to it).  The golden's inputs and initial parameters are drawn from seeds by
tests/golden/make_nb10_golden.py (draw_batch, draw_parameters), which also names the stored entries of a sampled tensor."""
import torch
import torch.nn.functional as F

from conv2d_f32_helpers import _golden_module, params64  # noqa: F401

STRIPE_WIDTH = 128 // 24
CONVS = ((0, 0, 1), (2, 0, 1), (4, 2, 1), (6, 2, 2))       # (module of self.conv, padding, stride); no ReLU after the last
G = _golden_module("nb10")


def stripe_plane64(stripe_start, h, w, width=STRIPE_WIDTH):
    """[B, 1, h, w] float64: 1 on columns start <= c < start + width (0 <= c < w), else 0."""
    start = torch.as_tensor(stripe_start).cpu().to(torch.int64).view(-1, 1, 1, 1)
    c = torch.arange(w).view(1, 1, 1, w)
    return ((c >= start) & (c < start + width)).double().expand(-1, 1, h, w).contiguous()


def input64(history, horizon):
    """[B, n_hist + 1, H, W] float64: the history frames, then the stripe plane of int(horizon * 5)."""
    history = torch.as_tensor(history).cpu().double()
    start = (torch.as_tensor(horizon).cpu().double() * STRIPE_WIDTH).trunc()
    return torch.cat((history, stripe_plane64(start, *history.shape[2:])), dim=1)


def forward64(p, batch):
    """y_hat [B, 1, (H - 1) // 2 + 1, (W - 1) // 2 + 1]."""
    out = input64(batch["HISTORICAL_SAT_IMAGES"], batch["FORECAST_HORIZON"])
    for i, pad, stride in CONVS:
        out = F.conv2d(out, p[f"conv.{i}.weight"], p[f"conv.{i}.bias"], stride=stride, padding=pad)
        if i != CONVS[-1][0]:
            out = F.relu(out)
    return out


def loss64(y_hat, target):
    return F.mse_loss(y_hat, torch.as_tensor(target).cpu().double().unsqueeze(1))


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
    """min over every ReLU unit of |pre-activation| / (tol * its sum of |products|), in float64.  A unit below 1 lies within
    the kernels' own tolerance of 0: two correct float32 implementations may gate it differently, and one such unit moves a
    gradient by about 1 / sqrt(units) of its norm (1e-3 here), so a fixture that holds one cannot pin gradients."""
    out = input64(batch["HISTORICAL_SAT_IMAGES"], batch["FORECAST_HORIZON"])
    worst = float("inf")
    with torch.no_grad():
        for i, pad, stride in CONVS[:-1]:
            w, b = p[f"conv.{i}.weight"], p[f"conv.{i}.bias"]
            z = F.conv2d(out, w, b, stride=stride, padding=pad)
            absz = F.conv2d(out.abs(), w.abs(), b.abs(), stride=stride, padding=pad)
            worst = min(worst, (z.abs() / (tol * absz)).min().item())
            out = F.relu(z)
    return worst
