"""GPU: notebook 16's max-pool Conv2d / ConvTranspose2d frame predictor (csrc/conv2d_ae_f32.hip, conv2d_functional,
models/conv2d/nb16_maxpool.py) against float64 on the CPU.

Tolerances are the project's own for exact-f32 conv kernels (conv2d_f32_helpers): ELEM_TOL per element relative to the
element's float64 sum of |products|, NORM_TOL relative norm for reductions.  A max pool is a selection, so its codes are
checked on their own (the picked entry is the window's float64 maximum within the tolerance) and the float64 gradients are
then routed through the kernel's own codes, every window included.  Against the golden fixture (torch float32 on the CPU,
another implementation's picks) the encoder gradients are held to ROUTED_TOL.

Parameters after three Adam steps (golden, case a): Adam's step is lr * m / (sqrt(v) + eps), about lr = 1e-3 per step
whatever the gradient's size.  Where |g| >> eps the step depends on the gradient only through ratios between steps, so a
relative gradient error d moves it by about lr * d: with d <= 1e-2 (ROUTED_TOL's order) that is 1e-5, which 99 % of the
elements of every tensor must meet.  The remaining elements are those whose gradient is ~ 0 and may take either sign in
two correct implementations: they may differ by 2 * lr per step, 3 * 2e-3 (+ 1e-6) in all.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nb16_reference as R
from conv2d_f32_helpers import ELEM_TOL, NORM_TOL, ROOT, _ops, _rel, _to, _within

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "nb16_small.npz")
DEAD = 255
# (batch, height, width): widths 128, 127, 44, 38, 36, 11 -- multiples and non-multiples of every tile extent
SHAPES = [(1, 128, 128), (1, 21, 127), (2, 44, 44), (3, 38, 38), (2, 36, 36), (2, 11, 11)]
# the Conv2d layers (plain and pooled) also at a size that takes the general Conv3d route (>= 32768 output positions)
CONV_SHAPES = SHAPES + [(3, 128, 128)]


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def _conv_params(g, c_out, c_in):
    return _randn(g, c_out, c_in, 3, 3, scale=(9 * c_in) ** -0.5), _randn(g, c_out, scale=0.1)


def _windows(z, ph, pw):
    n, c = z.shape[:2]
    z = z[:, :, :3 * ph, :3 * pw].reshape(n, c, ph, 3, pw, 3)
    return z.permute(0, 1, 2, 4, 3, 5).reshape(n, c, ph, pw, 9)


def _check_pool(y, codes, pre64, abs64, what):
    """pooled y and codes against float64 pre-activations: the pick and the value (as tests/test_gpu_exp001.py)."""
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


def _counts(g, n, h, w, integer_flow=False):
    hist = torch.randint(0, 1024, (n, 4, h, w), generator=g).to(torch.int16)
    flow = torch.randint(0, 1024, (n, h, w), generator=g).float()
    if not integer_flow:
        flow = flow + torch.rand(n, h, w, generator=g) * 0.5
    return hist, flow, _randn(g, n)


# ---- 1. each entry point against float64 -------------------------------------------------------------------------------
@pytest.mark.parametrize("n, h, w", SHAPES)
def test_counts_layer_against_float64(device, n, h, w):
    K = _ops()
    g = _g(100 + w)
    hist, flow, hor = _counts(g, n, h, w)
    wt, b = _conv_params(g, 16, 6)
    x64 = R.input64(hist, flow, hor)
    w64, b64 = wt.double(), b.double()
    ref = F.conv2d(x64, w64, b64)
    absref = F.conv2d(x64.abs(), w64.abs(), b64.abs())
    y = K.conv2d_ae_counts_fwd_f32(hist.to(device), flow.to(device), hor.to(device), wt.to(device), b.to(device))
    assert tuple(y.shape) == (n, 16, h - 2, w - 2)
    _within(y, ref.relu(), absref, what="counts forward")
    dy = _randn(g, n, 16, h - 2, w - 2)
    dw, db = K.conv2d_ae_counts_bwd_weight_f32(hist.to(device), flow.to(device), hor.to(device), dy.to(device),
                                               (16, 6, 3, 3))
    dw64 = torch.nn.grad.conv2d_weight(x64, (16, 6, 3, 3), dy.double())
    assert _rel(dw, dw64) <= NORM_TOL and _rel(db, dy.double().sum((0, 2, 3))) <= NORM_TOL


def test_counts_layer_int16_and_f32_inputs_give_identical_bits(device):
    K = _ops()
    g = _g(7)
    hist, flow, hor = _counts(g, 2, 38, 36, integer_flow=True)
    wt, b = _conv_params(g, 16, 6)
    args = [t.to(device) for t in (hor, wt, b)]
    dy = _randn(g, 2, 16, 36, 34).to(device)
    outs = []
    for hd, fd in ((torch.int16, torch.int16), (torch.float32, torch.float32), (torch.int16, torch.float32)):
        hi, fl = hist.to(device=device, dtype=hd), flow.to(device=device, dtype=fd)
        y = K.conv2d_ae_counts_fwd_f32(hi, fl, *args)
        dw, db = K.conv2d_ae_counts_bwd_weight_f32(hi, fl, args[0], dy, (16, 6, 3, 3))
        outs.append((y, dw, db))
    for other in outs[1:]:
        for a, c in zip(outs[0], other):
            assert torch.equal(a, c)


@pytest.mark.parametrize("c_in", [16, 32])
@pytest.mark.parametrize("n, h, w", CONV_SHAPES)
def test_conv_against_float64(device, c_in, n, h, w):
    K = _ops()
    g = _g(200 + w + c_in)
    x = _randn(g, n, c_in, h, w)
    wt, b = _conv_params(g, 32, c_in)
    x64, w64, b64 = x.double(), wt.double(), b.double()
    pre = F.conv2d(x64, w64, b64)
    absref = F.conv2d(x64.abs(), w64.abs(), b64.abs())
    xd, wd, bd = x.to(device), wt.to(device), b.to(device)
    y = K.conv2d_ae_fwd_f32(xd, wd, bd, relu=True)
    _within(y, pre.relu(), absref, what="forward relu")
    _within(K.conv2d_ae_fwd_f32(xd, wd, None, relu=False), pre - b64.view(1, -1, 1, 1), absref, what="forward plain")
    dy = _randn(g, *pre.shape)
    dy_gate, x_gate = _randn(g, *pre.shape), _randn(g, *x.shape)
    for use_dg, use_xg in ((True, True), (False, False), (True, False)):
        dyg = dy.double() * (dy_gate > 0) if use_dg else dy.double()
        dx64 = F.conv_transpose2d(dyg, w64)
        absdx = F.conv_transpose2d(dyg.abs(), w64.abs())
        if use_xg:
            dx64 = dx64 * (x_gate > 0)
        dx = K.conv2d_ae_bwd_data_f32(dy.to(device), dy_gate.to(device) if use_dg else None, wd,
                                      x_gate.to(device) if use_xg else None, tuple(x.shape))
        _within(dx, dx64, absdx, what=f"dx gates {use_dg} {use_xg}")
        dw, db = K.conv2d_ae_bwd_weight_f32(xd, dy.to(device), dy_gate.to(device) if use_dg else None, tuple(wt.shape))
        assert _rel(dw, torch.nn.grad.conv2d_weight(x64, tuple(wt.shape), dyg)) <= NORM_TOL
        assert _rel(db, dyg.sum((0, 2, 3))) <= NORM_TOL


# ---- 2. the fused pool: codes on their own, then float64 gradients routed through them -----------------------------
@pytest.mark.parametrize("n, h, w", CONV_SHAPES)
def test_pooled_conv_against_float64(device, n, h, w):
    K = _ops()
    g = _g(300 + w)
    x = _randn(g, n, 32, h, w)
    wt, b = _conv_params(g, 32, 32)
    b = b - 0.3                                   # some dead windows
    x64 = x.double().requires_grad_(True)
    w64, b64 = wt.double().requires_grad_(True), b.double().requires_grad_(True)
    z = F.conv2d(x64, w64, b64)
    z.retain_grad()
    absref = F.conv2d(x64.detach().abs(), w64.detach().abs(), b64.detach().abs())
    xd, wd, bd = x.to(device), wt.to(device), b.to(device)
    y, codes = K.conv2d_ae_pool_fwd_f32(xd, wd, bd)
    ph, pw = (h - 2) // 3, (w - 2) // 3
    assert tuple(y.shape) == (n, 32, ph, pw) and codes.dtype == torch.uint8 and tuple(codes.shape) == tuple(y.shape)
    _check_pool(y, codes, z.detach(), absref, "pool forward")
    dyp = _randn(g, n, 32, ph, pw)
    _pool_by_codes(z, codes).backward(dyp.double())
    absdx = F.conv_transpose2d(z.grad.abs(), w64.detach().abs())
    x_gate = _randn(g, *x.shape)
    dx = K.conv2d_ae_pool_bwd_data_f32(dyp.to(device), codes, wd, None, tuple(x.shape))
    _within(dx, x64.grad, absdx, what="pooled dx")
    dxg = K.conv2d_ae_pool_bwd_data_f32(dyp.to(device), codes, wd, x_gate.to(device), tuple(x.shape))
    _within(dxg, x64.grad * (x_gate > 0), absdx, what="pooled dx gated")
    dw, db = K.conv2d_ae_pool_bwd_weight_f32(xd, dyp.to(device), codes, tuple(wt.shape))
    assert _rel(dw, w64.grad) <= NORM_TOL and _rel(db, b64.grad) <= NORM_TOL


# ---- 3. ConvTranspose2d ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c_in, c_out", [(32, 32), (32, 16), (16, 16), (16, 1)])
@pytest.mark.parametrize("n, h, w", [(1, 40, 40), (2, 3, 126), (3, 10, 9), (2, 46, 46), (1, 1, 1)])
def test_conv_transpose_against_float64(device, c_in, c_out, n, h, w):
    K = _ops()
    g = _g(400 + w + c_in + c_out)
    x = _randn(g, n, c_in, h, w)
    wt = _randn(g, c_in, c_out, 3, 3, scale=(9 * c_in) ** -0.5)
    b = _randn(g, c_out, scale=0.1)
    xd, wd, bd = x.to(device), wt.to(device), b.to(device)
    x64 = x.double().requires_grad_(True)
    w64, b64 = wt.double().requires_grad_(True), b.double().requires_grad_(True)
    pre = F.conv_transpose2d(x64, w64, b64)
    absref = F.conv_transpose2d(x64.detach().abs(), w64.detach().abs(), b64.detach().abs())
    for relu in (True, False):
        y = K.convt2d_ae_fwd_f32(xd, wd, bd, relu=relu)
        assert tuple(y.shape) == (n, c_out, h + 2, w + 2)
        _within(y, pre.detach().relu() if relu else pre.detach(), absref, what=f"convT forward relu={relu}")
    _within(K.convt2d_ae_fwd_f32(xd, wd, None, relu=False), pre.detach() - b64.detach().view(1, -1, 1, 1), absref,
            what="convT forward without bias")
    dy, dy_gate, x_gate = _randn(g, *pre.shape), _randn(g, *pre.shape), _randn(g, *x.shape)
    for use_dg in (True, False):       # with and without a ReLU gate on dy
        dyg = dy.double() * (dy_gate > 0) if use_dg else dy.double()
        gate_d = dy_gate.to(device) if use_dg else None
        for t in (x64, w64, b64):
            t.grad = None
        pre.backward(dyg, retain_graph=True)
        absdx = F.conv2d(dyg.abs(), w64.detach().abs())
        dx = K.convt2d_ae_bwd_data_f32(dy.to(device), gate_d, wd, None, tuple(x.shape))
        _within(dx, x64.grad, absdx, what=f"convT dx gate={use_dg}")
        dxg = K.convt2d_ae_bwd_data_f32(dy.to(device), gate_d, wd, x_gate.to(device), tuple(x.shape))
        _within(dxg, x64.grad * (x_gate > 0), absdx, what=f"convT dx gated gate={use_dg}")
        dw, db = K.convt2d_ae_bwd_weight_f32(xd, dy.to(device), gate_d, tuple(wt.shape))
        assert tuple(dw.shape) == tuple(wt.shape) and tuple(db.shape) == (c_out,)
        assert _rel(dw, w64.grad) <= NORM_TOL, (use_dg, _rel(dw, w64.grad))
        assert _rel(db, b64.grad) <= NORM_TOL, (use_dg, _rel(db, b64.grad))


@pytest.mark.parametrize("dtype", [torch.int16, torch.float32])
@pytest.mark.parametrize("n, side", [(3, 18), (2, 17), (4, 48), (1, 1)])
def test_cropped_normalised_mse_against_float64(device, dtype, n, side):
    K = _ops()
    g = _g(500 + side)
    y_hat = _randn(g, n, side, side, scale=2.0)
    target = torch.randint(0, 1024, (n, side + 16, side + 16), generator=g).to(dtype)
    loss, grad = K.mse_crop_norm_f32(y_hat.to(device), target.to(device))
    t64 = R.normalise64(target)[..., 8:-8, 8:-8]
    d64 = y_hat.double() - t64
    ref = (d64 ** 2).mean()
    assert abs(loss.item() - ref.item()) <= 1e-5 * ref.item()
    count = n * side * side
    _within(grad, 2 * d64 / count, 2 * (y_hat.double().abs() + t64.abs()) / count, what="dy_hat")


# ---- 4. the model against the golden -----------------------------------------------------------------------------------
def _load_model(device, init):
    from predict_pv_yield_amd.models.conv2d.nb16_maxpool import LitAutoEncoder
    model = LitAutoEncoder()
    model.load_state_dict(init)
    return model.to(device)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_model_against_golden(device, tag):
    gold = np.load(GOLDEN)
    batch, init = R.golden_case(gold, tag)
    model = _load_model(device, init)
    dbatch = _to(batch, device)
    y_hat = model(dbatch)
    assert tuple(y_hat.shape) == tuple(gold[f"{tag}/y_hat"].shape)
    assert _rel(y_hat.detach(), gold[f"{tag}/y_hat"]) <= NORM_TOL
    opt = model.configure_optimizers()
    losses = []
    for step in range(3):
        opt.zero_grad(set_to_none=True)
        loss = model.training_step(dbatch, 0)
        loss.backward()
        if step == 0:
            for k, p in model.named_parameters():
                tol = R.ROUTED_TOL if k.startswith("encoder") else NORM_TOL
                err = _rel(p.grad, gold[f"{tag}/grad/{k}"])
                print(f"{tag} grad {k}: rel {err:.3e} (bound {tol})")
                assert err <= tol, (k, err)
        opt.step()
        losses.append(loss.item())
    for got, want in zip(losses, gold[f"{tag}/losses"]):
        assert abs(got - want) <= 1e-5 * want, (losses, gold[f"{tag}/losses"])
    if f"{tag}/step3/encoder_conv1.weight" not in gold.files:
        return                                     # case b stores losses only after the first step (fixture size)
    for k, p in model.named_parameters():
        want = torch.from_numpy(gold[f"{tag}/step3/{k}"]).double()
        err = (p.detach().cpu().double() - want).abs()
        moved = (want - init[k].double()).abs()
        q99 = err.flatten().sort().values[int(0.99 * (err.numel() - 1))].item()
        print(f"{tag} step3 {k}: max {err.max().item():.3e} 99% {q99:.3e} moved median {moved.median().item():.3e}")
        assert moved.median().item() >= 1e-4, k       # the fixture's parameters did move (three steps of lr = 1e-3)
        assert q99 <= 1e-5, (k, q99)
        assert err.max().item() <= 3 * 2e-3 + 1e-6, k


# ---- 5. full size ------------------------------------------------------------------------------------------------------
def _full_batch(seed, b=4, s=128):
    g = _g(seed)
    hist, flow, hor = _counts(g, b, s, s)
    t = (s - 8) // 3 + 24
    target = torch.randint(0, 1024, (b, t, t), generator=g).to(torch.int16)
    return {"HISTORICAL_SAT_IMAGES": hist, "OPTICAL_FLOW_PREDICTIONS": flow, "FORECAST_HORIZON": hor,
            "TARGET_SAT_IMAGE": target}


@pytest.mark.parametrize("b, s, out", [(4, 128, 48), (2, 11, 9)])
def test_full_size_forward_and_loss(device, b, s, out):
    """The notebook's size (B = 4, S = 128 -> [4, 1, 48, 48]) and the smallest image the model takes (one pool window)."""
    from predict_pv_yield_amd.models.conv2d.nb16_maxpool import LitAutoEncoder
    torch.manual_seed(5)
    model = LitAutoEncoder().to(device)
    batch = _full_batch(50, b, s)
    y_hat = model(_to(batch, device))
    assert tuple(y_hat.shape) == (b, 1, out, out)
    loss = model.training_step(_to(batch, device), 0)
    p = R.params64(model.state_dict(), requires_grad=False)
    y64 = R.forward64(p, batch)
    assert _rel(y_hat.detach(), y64) <= NORM_TOL
    ref = R.loss64(y64, batch["TARGET_SAT_IMAGE"]).item()
    assert abs(loss.item() - ref) <= 1e-5 * ref, (loss.item(), ref)


# ---- 6. determinism and HIP-graph replay ---------------------------------------------------------------------------
def _train(device, steps, seed=3, b=4):
    from predict_pv_yield_amd.models.conv2d.nb16_maxpool import LitAutoEncoder
    torch.manual_seed(seed)
    model = LitAutoEncoder().to(device)
    opt = model.configure_optimizers()
    losses = []
    for i in range(steps):
        batch = _to(_full_batch(60 + i, b=b), device)
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
    from predict_pv_yield_amd.graphs import GraphedTrainStep
    from predict_pv_yield_amd.models.conv2d.nb16_maxpool import LitAutoEncoder
    from predict_pv_yield_amd.optim import HipAdam
    batches = [_to(_full_batch(70 + s), device) for s in range(3)]

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
        for i in range(5):
            opt_e.zero_grad(set_to_none=True)
            loss = model_e.training_step(batches[i % 3], 0)
            loss.backward()
            opt_e.step()
            assert float(step(batches[i % 3])) == float(loss), f"step {i}"
        for p, q in zip(model_g.parameters(), model_e.parameters()):
            assert torch.equal(p, q)
    finally:
        step.close()


# ---- 7. Trainer.fit on the fake datamodule -------------------------------------------------------------------------
def test_trainer_fit_on_the_fake_datamodule(device, tmp_path):
    from predict_pv_yield_amd import lightning as pl
    from predict_pv_yield_amd.data.nb16_datamodule import Nb16DataModule
    from predict_pv_yield_amd.models.conv2d.nb16_maxpool import LitAutoEncoder

    class Recording(LitAutoEncoder):
        seen = []

        def log_dict(self, d, **kw):
            type(self).seen.extend((k, v.detach()) for k, v in d.items())
            return super().log_dict(d, **kw)

    Recording.seen = []
    torch.manual_seed(1)
    model = Recording()
    dm = Nb16DataModule(batch_size=4, n_train_data=3, n_val_data=1, n_super_batches=1)
    ckpt = pl.ModelCheckpoint(save_last=True, dirpath=str(tmp_path / "ck"))
    trainer = pl.Trainer(gpus=1, max_epochs=1, callbacks=[ckpt], log_every_n_steps=1)
    trainer.fit(model, datamodule=dm)
    batch = next(iter(dm.train_dataloader()))
    assert batch["HISTORICAL_SAT_IMAGES"].dtype == torch.int16 and tuple(batch["HISTORICAL_SAT_IMAGES"].shape) == (4, 4, 128, 128)
    assert batch["OPTICAL_FLOW_PREDICTIONS"].dtype == torch.float32 and tuple(batch["TARGET_SAT_IMAGE"].shape) == (4, 64, 64)
    assert float(batch["HISTORICAL_SAT_IMAGES"].float().max()) > 10.0          # raw counts, not normalised
    train = [float(v) for k, v in Recording.seen if k == "Loss/Train"]
    assert len(train) == 3 and all(np.isfinite(train)), train
    assert any(k == "Loss/Validation" for k, _ in Recording.seen)
    state = torch.load(ckpt.last_model_path)["state_dict"]
    assert list(state) == [f"{n}.{w}" for n in R.ENC + R.DEC for w in ("weight", "bias")]
    fresh = LitAutoEncoder()
    fresh.load_state_dict(state)
    for (k, p), q in zip(model.state_dict().items(), fresh.state_dict().values()):
        assert torch.equal(p.cpu(), q), k


def test_trainer_fit_with_hip_graph_matches_the_eager_fit(device):
    """`run.py ... +trainer.hip_graph=true`: Trainer(hip_graph=True) replays the step after its eager steps; more batches
    than those, same parameters and logged losses as the eager fit."""
    from predict_pv_yield_amd import lightning as pl
    from predict_pv_yield_amd.data.nb16_datamodule import Nb16DataModule
    from predict_pv_yield_amd.models.conv2d.nb16_maxpool import LitAutoEncoder
    dm = Nb16DataModule(batch_size=4, n_train_data=pl.Trainer.GRAPH_EAGER_STEPS + 3, n_val_data=1, n_super_batches=1)
    results = []
    for graph in (False, True):
        torch.manual_seed(2)
        model = LitAutoEncoder()
        trainer = pl.Trainer(gpus=1, max_epochs=1, hip_graph=graph, log_every_n_steps=1)
        trainer.fit(model, datamodule=dm)
        results.append(({k: v.detach().clone() for k, v in model.state_dict().items()}, dict(trainer.callback_metrics)))
    (sd_e, log_e), (sd_g, log_g) = results
    for k in sd_e:
        assert torch.equal(sd_e[k], sd_g[k]), k
    assert np.isfinite(float(log_g["Loss/Train_epoch"])) and float(log_g["Loss/Train_epoch"]) == float(log_e["Loss/Train_epoch"])


# ---- 8. refusals through the Python surface ------------------------------------------------------------------------
def test_refusals_raise_before_any_launch(device):
    K = _ops()
    z = lambda *s: torch.zeros(*s, device=device)      # noqa: E731
    with pytest.raises(RuntimeError, match="status -2"):
        K.conv2d_ae_fwd_f32(z(1, 32, 8, 130), z(32, 32, 3, 3), z(32))
    with pytest.raises(RuntimeError, match="status -2"):
        K.conv2d_ae_fwd_f32(z(1, 32, 8, 8), z(16, 32, 3, 3), z(16))
    with pytest.raises(RuntimeError, match="status -2"):
        K.conv2d_ae_counts_fwd_f32(z(1, 4, 10, 10).to(torch.int16), z(1, 10, 10), z(1), z(16, 6, 3, 3), z(16))
    with pytest.raises(ValueError, match="at least 5 x 5"):
        K.conv2d_ae_pool_fwd_f32(z(1, 32, 4, 9), z(32, 32, 3, 3), z(32))
    with pytest.raises(RuntimeError, match="status -2"):
        K.conv2d_ae_pool_fwd_f32(z(1, 16, 9, 9), z(32, 16, 3, 3), z(32))
    with pytest.raises(RuntimeError, match="status -2"):
        K.convt2d_ae_fwd_f32(z(1, 16, 8, 8), z(16, 32, 3, 3), z(32))
    with pytest.raises(RuntimeError, match="status -2"):
        K.convt2d_ae_fwd_f32(z(1, 32, 8, 127), z(32, 32, 3, 3), z(32))
    with pytest.raises(RuntimeError, match="target side"):
        K.mse_crop_norm_f32(z(2, 18, 18), z(2, 33, 33).to(torch.int16))
    with pytest.raises(TypeError):
        K.conv2d_ae_counts_fwd_f32(z(1, 4, 12, 12).double(), z(1, 12, 12), z(1), z(16, 6, 3, 3), z(16))
