"""GPU: the LitModel of experiments/002_cnn_processes_single_sat_image_then_rnn.py (Conv2d 17 -> 32 -> 32 -> 4 over every
satellite image, then the GRU encoder / decoder of experiment 003) on the Conv2d kernels of csrc/conv2d_f32.hip.

Tolerances.  The kernels multiply in exact f32 (one rounding per product, f32 accumulation) in a different summation order
from torch: an output element's error is then a few ulp of its sum of |products| (about 1e-7 of it per rounding at these
depths, K <= 288), so each element is held to 1e-6 of its own sum of |products|, computed alongside in float64.  The weight
gradients add up to 600 000 products per element: held to 1e-5 relative norm against float64.
The 32 -> 32 and 32 -> 4 layers' three passes are the record `conv2d` of tests/conv_family_checks.py, checked by its check_family.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_family_checks as C
from conv2d_f32_helpers import NORM_TOL, ROOT, _golden_module, _ops, _rel, _to, _within

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "exp002_small.npz")


# ---- the plain families' three passes: the records and the checker of tests/conv_family_checks.py ------------------------
@C.cases_of("conv2d", ids="{c_out}-{shape}")
def test_conv2d_entry_points_against_float64(device, fam, c_in, c_out, shape):
    C.check_family(_ops(), device, fam, c_in, c_out, shape)


# ---- layer 1: the 17-channel input built by the kernels -----------------------------------------------------------------
def _reference_input(sat, xc, yc, seq_len):
    """The reference's own tensor ops (experiments/002...py:140-162, 180-208), restated at any batch size, in float32."""
    n, width, height, _ = sat.shape
    s = height
    center_marker = torch.zeros((n, 1, width, height), dtype=torch.float32)
    half_width = s // 2
    center_marker[..., half_width - 2:half_width + 2, half_width - 2:half_width + 2] = 1
    pixel_range = (torch.arange(s) - 64) / 37
    pixel_range = pixel_range.unsqueeze(0).unsqueeze(0)
    pixel_x = pixel_range.unsqueeze(-2).expand(n, 1, s, -1)
    pixel_y = pixel_range.unsqueeze(-1).expand(n, 1, -1, s)
    x_coords = (xc - np.float32(309000)) / np.float32(316387.42073603)
    x_coords = x_coords.unsqueeze(1).expand(-1, width, -1).unsqueeze(1).repeat_interleave(repeats=seq_len, dim=0)
    y_coords = (yc - np.float32(519000)) / np.float32(406454.17945938)
    y_coords = y_coords.unsqueeze(-1).expand(-1, -1, height).unsqueeze(1).repeat_interleave(repeats=seq_len, dim=0)
    return torch.cat((sat.permute(0, 3, 1, 2), center_marker, x_coords, y_coords, pixel_x, pixel_y), dim=1)


def _coords_batch(b, t, s, seed):
    from predict_pv_yield_amd.data.exp002_datamodule import make_fake_exp002_batch
    batch = make_fake_exp002_batch(b, s, torch.Generator().manual_seed(seed), history_len=t - 2, forecast_len=1)
    return batch["sat_data"].reshape(b * t, s, s, 12), batch["sat_x_coords"], batch["sat_y_coords"]


@pytest.mark.parametrize("b,t,s", [(2, 19, 32), (1, 3, 5), (3, 2, 13)])
def test_coords_layer_against_the_reference_concatenation(device, b, t, s):
    K = _ops()
    sat, xc, yc = _coords_batch(b, t, s, seed=s)
    inp = _reference_input(sat, xc, yc, t).double()
    g = torch.Generator().manual_seed(5)
    wt = torch.randn(32, 17, 3, 3, generator=g) / 12.0
    bias = torch.randn(32, generator=g) * 0.1
    pre64 = F.conv2d(inp, wt.double(), bias.double())
    abs64 = F.conv2d(inp.abs(), wt.double().abs(), bias.double().abs())
    args = (sat.to(device), xc.to(device), yc.to(device))
    y = K.conv2d_coords_fwd_f32(*args, wt.to(device), bias.to(device), t)
    _within(y, pre64.relu(), abs64, what="coords forward")

    dy = torch.randn(pre64.shape, generator=g).double()
    dw64 = torch.nn.grad.conv2d_weight(inp, wt.shape, dy)
    dw, db = K.conv2d_coords_bwd_weight_f32(*args, dy.float().to(device), t, tuple(wt.shape))
    assert _rel(dw, dw64) <= NORM_TOL and _rel(db, dy.sum(dim=(0, 2, 3))) <= NORM_TOL


def test_synthesised_channels_are_bit_identical(device):
    """A weight that selects one input channel at one tap (+1 or -1, zero bias) returns that channel exactly through the
    ReLU: compared bit for bit with the reference's float32 construction.  The nine taps together cover the whole plane,
    its border rows and columns included."""
    K = _ops()
    b, t, s = 2, 3, 32
    sat, xc, yc = _coords_batch(b, t, s, seed=7)
    inp = _reference_input(sat, xc, yc, t)
    args = (sat.to(device), xc.to(device), yc.to(device))
    for ch in range(17):
        for tap in range(9):
            kh, kw = divmod(tap, 3)
            for sign in (1.0, -1.0):
                wt = torch.zeros(32, 17, 3, 3)
                wt[0, ch, kh, kw] = sign
                y = K.conv2d_coords_fwd_f32(*args, wt.to(device), torch.zeros(32, device=device), t).cpu()
                want = (sign * inp[:, ch, kh:kh + s - 2, kw:kw + s - 2]).relu()
                assert torch.equal(y[:, 0], want), f"channel {ch} tap {tap} sign {sign}"
                assert not y[:, 1:].any()


# ---- the whole model ----------------------------------------------------------------------------------------------------
def _model_from(params_np, device):
    from predict_pv_yield_amd.models.conv2d.exp002 import LitModel
    model = LitModel()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params_np.items()})
    return model.to(device)


def test_model_against_the_reference_golden(device):
    gm = _golden_module("exp002")
    gold = np.load(GOLDEN)
    from predict_pv_yield_amd.models.conv2d.exp002 import LitModel
    shapes = {k: tuple(v.shape) for k, v in LitModel().state_dict().items()}
    assert sorted(shapes) == list(gold["param_names"])
    init = gm.draw_parameters(shapes)
    model = _model_from(init, device)
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
        if k in gm.SAMPLED:
            idx = torch.from_numpy(gm.sample_index(g.numel()))
            norm = float(gold[f"grad/{k}/norm"])
            assert abs(g.double().norm().item() - norm) <= 1e-4 * norm, k
            # |sum error| <= sqrt(numel) x the error norm
            assert abs(g.double().sum().item() - float(gold[f"grad/{k}/sum"])) <= 1e-4 * norm * g.numel() ** 0.5, k
            g, a = g.reshape(-1)[idx], a.reshape(-1)[idx]
            g_gold = torch.from_numpy(gold[f"grad/{k}/sample"])
            a_gold = torch.from_numpy(gold[f"after/{k}/sample"])
        else:
            g_gold, a_gold = torch.from_numpy(gold[f"grad/{k}"]), torch.from_numpy(gold[f"after/{k}"])
        assert _rel(g, g_gold) <= 1e-4, (k, _rel(g, g_gold))
        # Adam's first step is lr * g / (|g| + eps), eps = 1e-8: where |g| >= 1e-6 a gradient error d moves it by at most
        # lr * (d / |g|) * (eps / |g|) <= 1e-2 lr * (d / |g|), i.e. well inside 1e-3 lr; smaller gradients may step anywhere
        # in [-lr, lr]
        err = (a - a_gold).abs()
        big = g_gold.abs() >= 1e-6
        assert err[big].max().item() <= 1e-6 if big.any() else True, k
        assert err.max().item() <= 2e-3 + 1e-6, k


def _forward64(params, batch, forecast_len=12, history_len=6):
    """float64 CPU restatement of experiments/002's forward at any batch size (reference ops, reference order)."""
    p = {k: torch.as_tensor(v).double() for k, v in params.items()}
    sat = batch["sat_data"]
    b, t, s = sat.shape[0], sat.shape[1], sat.shape[2]
    inp = _reference_input(sat.reshape(b * t, s, s, 12).float(), batch["sat_x_coords"].float(),
                           batch["sat_y_coords"].float(), t).double()
    out = F.relu(F.conv2d(inp, p["sat_conv1.weight"], p["sat_conv1.bias"]))
    out = F.relu(F.conv2d(out, p["sat_conv2.weight"], p["sat_conv2.bias"]))
    out = F.relu(F.conv2d(out, p["sat_conv3.weight"], p["sat_conv3.bias"]))
    out = F.relu(F.linear(out.reshape(b * t, -1), p["fc1.weight"], p["fc1.bias"]))
    emb = p["pv_system_id_embedding.weight"][batch["pv_system_row_number"].repeat_interleave(t)]
    out = torch.cat((out, emb), dim=1)
    for i in (2, 3, 4, 5):
        out = F.relu(F.linear(out, p[f"fc{i}.weight"], p[f"fc{i}.bias"]))
    out = out.reshape(b, t, 8)
    nwp = batch["nwp"].double().permute(0, 2, 1, 3, 4).reshape(b, t, -1)
    rnn_input = torch.cat((out, nwp) + tuple(batch[k].double().unsqueeze(-1) for k in
                                             ("hour_of_day_sin", "hour_of_day_cos", "day_of_year_sin", "day_of_year_cos")), dim=2)
    enc_in = torch.cat((rnn_input[:, :history_len + 1], batch["pv_yield"][:, :history_len + 1].double().unsqueeze(-1)), dim=2)

    def gru(x, prefix, h0=None):
        mod = torch.nn.GRU(x.shape[2], 16, num_layers=2, batch_first=True).double()
        mod.load_state_dict({k[len(prefix) + 1:]: v for k, v in p.items() if k.startswith(prefix + ".")})
        return mod(x, h0)

    _, h = gru(enc_in, "encoder_rnn")
    dec, _ = gru(rnn_input[:, -forecast_len:], "decoder_rnn", h)
    dec = F.relu(F.linear(dec, p["decoder_fc1.weight"], p["decoder_fc1.bias"]))
    return F.linear(dec, p["decoder_fc2.weight"], p["decoder_fc2.bias"])[..., 0]


@pytest.mark.parametrize("b", [1, 5, 32])
def test_any_batch_size_against_a_float64_restatement(device, b):
    from predict_pv_yield_amd.data.exp002_datamodule import make_fake_exp002_batch
    from predict_pv_yield_amd.models.conv2d.exp002 import LitModel
    torch.manual_seed(b)
    model = LitModel().to(device)
    batch = make_fake_exp002_batch(b, 32, torch.Generator().manual_seed(100 + b))
    y_hat = model(_to(batch, device))
    assert tuple(y_hat.shape) == (b, 12)
    params64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    ref = _forward64(params64, batch)
    assert _rel(y_hat.detach(), ref.detach()) <= 1e-5
    y = batch["pv_yield"][:, -12:]
    loss = model.training_step(_to(batch, device), 0)
    loss64 = (ref - y.double()).abs().mean()
    assert abs(loss.item() - loss64.item()) <= 1e-5 * loss64.item()
    loss.backward()
    loss64.backward()
    named = dict(model.named_parameters())
    for k, v in params64.items():
        if v.grad is None or v.grad.abs().max() == 0:
            continue
        assert _rel(named[k].grad, v.grad) <= 1e-4, (k, _rel(named[k].grad, v.grad))


def _train(device, steps, seed=3):
    from predict_pv_yield_amd.data.exp002_datamodule import make_fake_exp002_batch
    from predict_pv_yield_amd.models.conv2d.exp002 import LitModel
    torch.manual_seed(seed)
    model = LitModel().to(device)
    opt = model.configure_optimizers()
    losses = []
    for i in range(steps):
        batch = _to(make_fake_exp002_batch(32, 32, torch.Generator().manual_seed(i)), device)
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
    from predict_pv_yield_amd.data.exp002_datamodule import make_fake_exp002_batch
    from predict_pv_yield_amd.graphs import GraphedTrainStep
    from predict_pv_yield_amd.models.conv2d.exp002 import LitModel
    from predict_pv_yield_amd.optim import HipAdam
    batches = [_to(make_fake_exp002_batch(32, 32, torch.Generator().manual_seed(s)), device) for s in range(3)]

    def make(capturable):
        torch.manual_seed(11)
        model = LitModel().to(device)
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


def test_cli_fast_dev_run(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run.py"), "model=exp002_cnn_rnn", "datamodule=exp002_fake",
                        "trainer.fast_dev_run=true"], cwd=str(tmp_path), env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def test_public_conv_functions_gate_their_own_gradient(device):
    """coords_conv2d_relu / conv2d_relu with an output used twice (two consumers, neither a conv): the weight and bias
    gradients equal float64 autograd's, so the public functions never assume a pre-gated incoming gradient."""
    from predict_pv_yield_amd.conv2d_functional import conv2d_relu, coords_conv2d_relu
    b, t, s = 2, 3, 12
    sat, xc, yc = _coords_batch(b, t, s, seed=9)
    g = torch.Generator().manual_seed(9)
    w1, b1 = torch.randn(32, 17, 3, 3, generator=g) / 12.0, torch.randn(32, generator=g) * 0.1
    w2, b2 = torch.randn(4, 32, 3, 3, generator=g) / 17.0, torch.randn(4, generator=g) * 0.1
    r1 = torch.randn(b * t, 32, s - 2, s - 2, generator=g)
    r2 = torch.randn(b * t, 4, s - 4, s - 4, generator=g)

    def loss_of(y1, y2, rr1, rr2):
        return (y1 * rr1).sum() + (y1 ** 2).sum() * 0.01 + (y2 * rr2).sum() + (y2 ** 2).sum() * 0.01

    params = [p.to(device).requires_grad_(True) for p in (w1, b1, w2, b2)]
    y1 = coords_conv2d_relu(sat.to(device), xc.to(device), yc.to(device), params[0], params[1], t)
    y2 = conv2d_relu(y1, params[2], params[3], x_is_relu_output=True)
    loss_of(y1, y2, r1.to(device), r2.to(device)).backward()

    p64 = [p.double().requires_grad_(True) for p in (w1, b1, w2, b2)]
    z1 = F.relu(F.conv2d(_reference_input(sat, xc, yc, t).double(), p64[0], p64[1]))
    z2 = F.relu(F.conv2d(z1, p64[2], p64[3]))
    loss_of(z1, z2, r1.double(), r2.double()).backward()
    for got, want in zip(params, p64):
        assert _rel(got.grad, want.grad) <= NORM_TOL, _rel(got.grad, want.grad)
