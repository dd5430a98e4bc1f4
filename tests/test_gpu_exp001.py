"""GPU: the LitAutoEncoder of experiments/001_CNN_concat_all_timesteps_as_channels.py (7 stacked HRV frames + 5 synthesised
channels, Conv2d 12 -> 144 -> 144 -> 144 with MaxPool2d(3) after the first two, then fc1..fc5) on the kernels of
csrc/conv2d_pool_f32.hip.

Tolerances (as tests/test_gpu_exp002.py).  The kernels multiply in exact f32 with f32 accumulation in another summation
order than torch: each output element is held to 1e-6 of its own sum of |products| (computed alongside in float64), each
weight / bias gradient to 1e-5 relative norm against float64.
The plain 144 -> 144 layer's three passes are the record `conv2d144` of tests/conv_family_checks.py, checked by its check_family.
Pool routing.  Where two entries of a window lie closer than that rounding, f32 may pick either as the maximum, and the
gradient follows the pick.  So the codes are checked on their own -- the picked entry is within the tolerance of the float64
maximum, dead windows have a maximum within the tolerance of <= 0 -- and the float64 gradients are then routed through the
kernel's own codes.  Against the reference's golden, computed with torch CPU's picks, the two gradients below a pool
(sat_conv1, sat_conv2) are held to ROUTED_TOL instead: one differing pick among the ~10^5 windows moves them by ~1e-3.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_family_checks as C
from conv2d_f32_helpers import ELEM_TOL, NORM_TOL, ROOT, _golden_module, _ops, _rel, _to, _within

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "exp001_small.npz")
ROUTED_TOL = 2e-2    # gradients below a pool against another implementation's picks (golden only)
DEAD = 255


def _windows(z, ph, pw):
    """[N, C, >= 3ph, >= 3pw] -> [N, C, ph, pw, 9] in row-major window order."""
    n, c = z.shape[:2]
    z = z[:, :, :3 * ph, :3 * pw].reshape(n, c, ph, 3, pw, 3)
    return z.permute(0, 1, 2, 4, 3, 5).reshape(n, c, ph, pw, 9)


def _check_pool(y, codes, pre64, abs64, what):
    """pooled y and codes against float64 pre-activations; returns nothing, asserts the pick and the value."""
    ph, pw = codes.shape[2:]
    zc, ac = _windows(pre64, ph, pw), _windows(abs64, ph, pw)
    tol = ELEM_TOL * ac.amax(-1)
    m = zc.amax(-1)
    codes = codes.cpu().long()
    live = codes != DEAD
    assert ((codes <= 8) | ~live).all(), what
    assert (m[~live] <= tol[~live]).all(), f"{what}: a dead window has a positive maximum"
    assert (m[live] >= -tol[live]).all(), f"{what}: a live window has a negative maximum"
    picked = zc.gather(-1, codes.clamp(max=8).unsqueeze(-1)).squeeze(-1)
    assert ((m - picked)[live] <= 2 * tol[live]).all(), f"{what}: the code does not pick the maximum"
    _within(y, m.relu(), ac.amax(-1), what=what)
    assert (y.cpu()[~live] == 0).all()


def _pool_by_codes(z, codes):
    """relu(max_pool2d(z, 3)) in float64 with the window picks of `codes` (autograd routes through them)."""
    ph, pw = codes.shape[2:]
    codes = codes.cpu().long()
    live = codes != DEAD
    picked = _windows(z, ph, pw).gather(-1, codes.clamp(max=8).unsqueeze(-1)).squeeze(-1)
    return torch.where(live, picked, torch.zeros_like(picked))


def _stacked_input(sat, xc, yc, n_frames):
    """The reference's own tensor ops (experiments/001...py:266-301) restated at any batch size, in float32."""
    sat_data = sat[:, :n_frames]
    batch_size, seq_len, width, height, n_chans = sat_data.shape
    sat_data = sat_data.permute(0, 2, 3, 4, 1).reshape(batch_size, width, height, seq_len * n_chans).permute(0, 3, 1, 2)
    center_marker = torch.zeros((batch_size, 1, width, height), dtype=torch.float32)
    half_width = width // 2
    center_marker[..., half_width - 2:half_width + 2, half_width - 2:half_width + 2] = 1
    x_coords = xc - np.float32(309000)
    x_coords = x_coords / np.float32(316387.42073603)
    x_coords = x_coords.unsqueeze(1).expand(-1, width, -1).unsqueeze(1)
    y_coords = yc - np.float32(519000)
    y_coords = y_coords / np.float32(406454.17945938)
    y_coords = y_coords.unsqueeze(-1).expand(-1, -1, height).unsqueeze(1)
    pixel_range = (torch.arange(width) - 64) / 37
    pixel_range = pixel_range.unsqueeze(0).unsqueeze(0)
    pixel_x = pixel_range.unsqueeze(-2).expand(batch_size, 1, width, -1)
    pixel_y = pixel_range.unsqueeze(-1).expand(batch_size, 1, -1, height)
    return torch.cat((sat_data, center_marker, x_coords, y_coords, pixel_x, pixel_y), dim=1)


def _sat_batch(b, t, s, seed):
    from predict_pv_yield_amd.data.exp001_datamodule import make_fake_exp001_batch
    batch = make_fake_exp001_batch(b, s, torch.Generator().manual_seed(seed), history_len=t - 2, forecast_len=1)
    return batch["sat_data"], batch["sat_x_coords"], batch["sat_y_coords"]


# ---- entry points against float64 torch.nn.functional -------------------------------------------------------------------
POOL_SHAPES = [(2, 42, 42), (1, 40, 40), (2, 41, 41), (1, 43, 44), (1, 5, 5), (3, 8, 13)]


@pytest.mark.parametrize("n,h,w", POOL_SHAPES)
def test_pooled_layer_against_float64(device, n, h, w):
    K = _ops()
    g = torch.Generator().manual_seed(n * 1000 + h * 10 + w)
    x = torch.randn(n, 144, h, w, generator=g).relu()               # a pooled ReLU output, as in the model
    wt = torch.randn(144, 144, 3, 3, generator=g) / 36.0
    b = torch.randn(144, generator=g) * 0.1
    x64, w64, b64 = x.double(), wt.double(), b.double()
    xd, wd, bd = x.to(device), wt.to(device), b.to(device)

    pre64 = F.conv2d(x64, w64, b64)
    abs64 = F.conv2d(x64.abs(), w64.abs(), b64.abs())
    y, codes = K.conv2d144_pool_fwd_f32(xd, wd, bd)
    assert tuple(y.shape) == tuple(codes.shape) == (n, 144, (h - 2) // 3, (w - 2) // 3)
    _check_pool(y, codes, pre64, abs64, "pooled forward")

    # backward through the kernel's own picks
    dyp = torch.randn(y.shape, generator=g)
    xr = x64.clone().requires_grad_(True)
    wr, br = w64.clone().requires_grad_(True), b64.clone().requires_grad_(True)
    (_pool_by_codes(F.conv2d(xr, wr, br), codes) * dyp.double()).sum().backward()
    dyd = dyp.to(device)
    dx = K.conv2d144_pool_bwd_data_f32(dyd, codes, wd, None, tuple(x.shape))
    z0 = torch.zeros_like(pre64).requires_grad_(True)      # |dz| through the same picks, for the bound
    (_pool_by_codes(z0, codes) * dyp.double().abs()).sum().backward()
    dx_abs = torch.nn.grad.conv2d_input(x.shape, w64.abs(), z0.grad)
    _within(dx, xr.grad, dx_abs, what="pooled dgrad")
    dxg = K.conv2d144_pool_bwd_data_f32(dyd, codes, wd, xd, tuple(x.shape))
    _within(dxg, xr.grad * (x64 > 0), dx_abs, what="pooled dgrad, gated")
    dw, db = K.conv2d144_pool_bwd_weight_f32(xd, dyd, codes, tuple(wt.shape))
    assert _rel(dw, wr.grad) <= NORM_TOL and _rel(db, br.grad) <= NORM_TOL, (_rel(dw, wr.grad), _rel(db, br.grad))


@pytest.mark.parametrize("b,t,s,n_frames", [(2, 19, 128, 7), (1, 3, 17, 3), (3, 9, 10, 7), (1, 8, 5, 1)])
def test_first_layer_against_the_reference_stacking(device, b, t, s, n_frames):
    K = _ops()
    sat, xc, yc = _sat_batch(b, t, s, seed=s + t)
    inp = _stacked_input(sat, xc, yc, n_frames).double()
    g = torch.Generator().manual_seed(5)
    wt = torch.randn(144, n_frames + 5, 3, 3, generator=g) / 10.0
    bias = torch.randn(144, generator=g) * 0.1
    pre64 = F.conv2d(inp, wt.double(), bias.double())
    abs64 = F.conv2d(inp.abs(), wt.double().abs(), bias.double().abs())
    args = (sat.to(device), xc.to(device), yc.to(device))
    y, codes = K.conv2d144_sat_pool_fwd_f32(*args, wt.to(device), bias.to(device), n_frames)
    _check_pool(y, codes, pre64, abs64, "first layer")

    # frames >= n_frames are not read: changing them leaves the output bit-identical
    sat2 = sat.clone()
    sat2[:, n_frames:] = torch.randn(sat2[:, n_frames:].shape, generator=g) * 100.0
    y2, codes2 = K.conv2d144_sat_pool_fwd_f32(sat2.to(device), *args[1:], wt.to(device), bias.to(device), n_frames)
    assert torch.equal(y, y2) and torch.equal(codes, codes2)

    dyp = torch.randn(y.shape, generator=g)
    wr, br = wt.double().requires_grad_(True), bias.double().requires_grad_(True)
    (_pool_by_codes(F.conv2d(inp, wr, br), codes) * dyp.double()).sum().backward()
    dw, db = K.conv2d144_sat_pool_bwd_weight_f32(*args, dyp.to(device), codes, n_frames)
    assert _rel(dw, wr.grad) <= NORM_TOL and _rel(db, br.grad) <= NORM_TOL, (_rel(dw, wr.grad), _rel(db, br.grad))


def test_ties_go_to_the_first_window_position_and_dead_windows_pass_nothing(device):
    """A constant input makes all nine pre-activations of every window equal: positive channels pick position 0, channels
    at or below 0 are dead (pooled 0, no gradient)."""
    K = _ops()
    n, h, w = 2, 14, 17
    x = torch.ones(n, 144, h, w)
    wt = torch.zeros(144, 144, 3, 3)
    b = torch.linspace(-1.0, 1.0, 144)                  # z = bias everywhere; one channel exactly 0 (dead)
    b[70] = 0.0
    y, codes = K.conv2d144_pool_fwd_f32(x.to(device), wt.to(device), b.to(device))
    codes = codes.cpu()
    pos = b > 0
    assert (codes[:, pos] == 0).all() and (codes[:, ~pos] == DEAD).all()
    assert torch.equal(y.cpu(), b.clamp(min=0)[None, :, None, None].expand_as(y.cpu()))
    dyp = torch.randn(y.shape, generator=torch.Generator().manual_seed(1))
    dz = torch.zeros(n, 144, h - 2, w - 2)
    dz[:, :, 0:3 * 4:3, 0:3 * 5:3] = dyp * pos[None, :, None, None]      # the first position of each window
    dw, db = K.conv2d144_pool_bwd_weight_f32(x.to(device), dyp.to(device), codes.to(device), tuple(wt.shape))
    assert _rel(dw, torch.nn.grad.conv2d_weight(x.double(), wt.shape, dz.double())) <= NORM_TOL
    assert _rel(db, dz.double().sum((0, 2, 3))) <= NORM_TOL
    assert (db.cpu()[~pos] == 0).all()
    wt2 = torch.randn(144, 144, 3, 3, generator=torch.Generator().manual_seed(2))
    dx = K.conv2d144_pool_bwd_data_f32(dyp.to(device), codes.to(device), wt2.to(device), None, (n, 144, h, w))
    _within(dx, torch.nn.grad.conv2d_input((n, 144, h, w), wt2.double(), dz.double()),
            torch.nn.grad.conv2d_input((n, 144, h, w), wt2.double().abs(), dz.double().abs()), what="tie dgrad")


# ---- the plain families' three passes: the records and the checker of tests/conv_family_checks.py ------------------------
@C.cases_of("conv2d144", ids="{shape}")
def test_plain_layer_against_float64(device, fam, c_in, c_out, shape):
    C.check_family(_ops(), device, fam, c_in, c_out, shape)


# ---- the whole model ----------------------------------------------------------------------------------------------------
def _model_from(params_np, device):
    from predict_pv_yield_amd.models.conv2d.exp001 import LitAutoEncoder
    model = LitAutoEncoder()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params_np.items()})
    return model.to(device)


def test_model_against_the_reference_golden(device):
    gm = _golden_module("exp001")
    gold = np.load(GOLDEN)
    from predict_pv_yield_amd.models.conv2d.exp001 import LitAutoEncoder
    shapes = {k: tuple(v.shape) for k, v in LitAutoEncoder().state_dict().items()}
    assert sorted(shapes) == list(gold["param_names"])
    model = _model_from(gm.draw_parameters(shapes), device)
    batch = _to({k: torch.from_numpy(v) for k, v in gm.draw_batch().items()}, device)

    opt = model.configure_optimizers()
    opt.zero_grad(set_to_none=True)
    y_hat = model(batch)
    assert tuple(y_hat.shape) == (2, 12)
    assert _rel(y_hat.detach(), gold["y_hat"]) <= 1e-5
    y = batch["pv_yield"][:, -12:]
    mse = ((y_hat.detach().double() - y.double()) ** 2).mean().item()
    assert abs(mse - float(gold["mse"])) <= 1e-5 * float(gold["mse"])
    loss = model.training_step(batch, 0)
    assert abs(loss.item() - float(gold["nmae"])) <= 1e-5 * float(gold["nmae"])
    loss.backward()
    grads = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()}
    opt.step()
    for k, p in model.named_parameters():
        g, a = grads[k], p.detach().cpu()
        tol = ROUTED_TOL if k.startswith(("sat_conv1.", "sat_conv2.")) else 1e-4
        if gm.sampled(g.numel()):
            idx = torch.from_numpy(gm.sample_index(g.numel()))
            norm = float(gold[f"grad/{k}/norm"])
            assert abs(g.double().norm().item() - norm) <= tol * norm, k
            assert abs(g.double().sum().item() - float(gold[f"grad/{k}/sum"])) <= tol * norm * g.numel() ** 0.5, k
            g, a = g.reshape(-1)[idx], a.reshape(-1)[idx]
            g_gold = torch.from_numpy(gold[f"grad/{k}/sample"])
            a_gold = torch.from_numpy(gold[f"after/{k}/sample"])
        else:
            g_gold, a_gold = torch.from_numpy(gold[f"grad/{k}"]), torch.from_numpy(gold[f"after/{k}"])
        assert _rel(g, g_gold) <= tol, (k, _rel(g, g_gold))
        # Adam's first step is lr * g / (|g| + eps): where |g| >= 1e-6 a relative gradient error d moves it by about
        # lr * d * eps / |g| (tiny); smaller gradients may step anywhere in [-lr, lr]
        err = (a - a_gold).abs()
        big = g_gold.abs() >= 1e-6
        if tol == 1e-4 and big.any():
            assert err[big].max().item() <= 1e-6, k
        assert err.max().item() <= 2e-3 + 1e-6, k


def _forward64(model, batch, device, history_len=6):
    """float64 CPU restatement of experiments/001's forward (reference ops, reference order) from the model's parameters,
    the pools routed through the kernels' own picks (see the module docstring).  Returns (y_hat64, params64)."""
    K = _ops()
    p = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.named_parameters()}
    n_frames = history_len + 1
    sat, xc, yc = batch["sat_data"], batch["sat_x_coords"], batch["sat_y_coords"]
    b = sat.shape[0]
    sd = {k: v.to(device) for k, v in (("sat", sat), ("xc", xc), ("yc", yc))}
    y1, codes1 = K.conv2d144_sat_pool_fwd_f32(sd["sat"], sd["xc"], sd["yc"], model.sat_conv1.weight.detach(),
                                              model.sat_conv1.bias.detach(), n_frames)
    _, codes2 = K.conv2d144_pool_fwd_f32(y1, model.sat_conv2.weight.detach(), model.sat_conv2.bias.detach())
    inp = _stacked_input(sat.cpu().float(), xc.cpu().float(), yc.cpu().float(), n_frames).double()
    out = _pool_by_codes(F.conv2d(inp, p["sat_conv1.weight"], p["sat_conv1.bias"]), codes1)
    out = _pool_by_codes(F.conv2d(out, p["sat_conv2.weight"], p["sat_conv2.bias"]), codes2)
    out = F.relu(F.conv2d(out, p["sat_conv3.weight"], p["sat_conv3.bias"]))
    out = F.relu(F.linear(out.reshape(b, -1), p["fc1.weight"], p["fc1.bias"]))
    c = {k: v.cpu() for k, v in batch.items()}
    out = torch.cat((out, c["pv_yield"][:, :n_frames].double(), c["nwp"].double().reshape(b, -1),
                     c["hour_of_day_sin"].double(), c["hour_of_day_cos"].double(), c["day_of_year_sin"].double(),
                     c["day_of_year_cos"].double(), p["pv_system_id_embedding.weight"][c["pv_system_row_number"]]), dim=1)
    for i in (2, 3, 4, 5):
        out = F.relu(F.linear(out, p[f"fc{i}.weight"], p[f"fc{i}.bias"]))
    return out, p


@pytest.mark.parametrize("b", [1, 3, 32])
def test_batch_sizes_against_a_float64_restatement(device, b):
    from predict_pv_yield_amd.data.exp001_datamodule import make_fake_exp001_batch
    from predict_pv_yield_amd.models.conv2d.exp001 import LitAutoEncoder
    torch.manual_seed(b)
    model = LitAutoEncoder().to(device)
    batch = _to(make_fake_exp001_batch(b, 128, torch.Generator().manual_seed(100 + b)), device)
    y_hat = model(batch)
    assert tuple(y_hat.shape) == (b, 12)
    ref, p64 = _forward64(model, batch, device)
    assert _rel(y_hat.detach(), ref.detach()) <= 1e-5
    y = batch["pv_yield"][:, -12:]
    loss = model.training_step(batch, 0)
    loss64 = (ref - y.cpu().double()).abs().mean()
    assert abs(loss.item() - loss64.item()) <= 1e-5 * loss64.item()
    loss.backward()
    loss64.backward()
    for k, param in model.named_parameters():
        want = p64[k].grad
        if want is None or want.abs().max() == 0:
            continue
        assert _rel(param.grad, want) <= 1e-4, (k, _rel(param.grad, want))


def _train(device, steps, seed=3, b=8):
    from predict_pv_yield_amd.data.exp001_datamodule import make_fake_exp001_batch
    from predict_pv_yield_amd.models.conv2d.exp001 import LitAutoEncoder
    torch.manual_seed(seed)
    model = LitAutoEncoder().to(device)
    opt = model.configure_optimizers()
    losses = []
    for i in range(steps):
        batch = _to(make_fake_exp001_batch(b, 128, torch.Generator().manual_seed(i)), device)
        opt.zero_grad(set_to_none=True)
        loss = model.training_step(batch, i)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    return model, losses


def test_train_steps_are_deterministic(device):
    m1, l1 = _train(device, 3)
    m2, l2 = _train(device, 3)
    assert l1 == l2
    for (k, p), q in zip(m1.named_parameters(), m2.parameters()):
        assert torch.equal(p, q), k


def test_train_step_replays_as_a_hip_graph(device):
    from predict_pv_yield_amd.data.exp001_datamodule import make_fake_exp001_batch
    from predict_pv_yield_amd.graphs import GraphedTrainStep
    from predict_pv_yield_amd.models.conv2d.exp001 import LitAutoEncoder
    from predict_pv_yield_amd.optim import HipAdam
    batches = [_to(make_fake_exp001_batch(32, 128, torch.Generator().manual_seed(s)), device) for s in range(3)]

    def make(capturable):
        torch.manual_seed(11)
        model = LitAutoEncoder().to(device)
        return model, HipAdam(model.parameters(), lr=0.001, capturable=capturable)

    model_e, opt_e = make(False)
    model_g, opt_g = make(True)
    step = GraphedTrainStep(model_g, opt_g, batches[0], warmup=2)
    try:
        for _ in range(2):
            opt_e.zero_grad(set_to_none=True)
            model_e.training_step(batches[0], 0).backward()
            opt_e.step()
        for i in range(4):
            opt_e.zero_grad(set_to_none=True)
            loss = model_e.training_step(batches[i % 3], 0)
            loss.backward()
            opt_e.step()
            assert float(step(batches[i % 3])) == float(loss), f"step {i}"
        for p, q in zip(model_g.parameters(), model_e.parameters()):
            assert torch.equal(p, q)
    finally:
        step.close()


def test_forward_memory_stays_small(device):
    """B = 32 with autograd on: the unfused conv1 activation alone would be 32 x 144 x 126 x 126 x 4 B = 292 MB."""
    from predict_pv_yield_amd.data.exp001_datamodule import make_fake_exp001_batch
    from predict_pv_yield_amd.models.conv2d.exp001 import LitAutoEncoder
    model = LitAutoEncoder().to(device)
    batch = _to(make_fake_exp001_batch(32, 128, torch.Generator().manual_seed(0)), device)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = model.training_step(batch, 0)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < 128 << 20, (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    loss.backward()


def test_cli_fast_dev_run(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run.py"), "model=exp001_cnn", "datamodule=exp001_fake",
                        "trainer.fast_dev_run=true"], cwd=str(tmp_path), env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
