"""GPU: the four-input first layer and the stride-1 horizon ConvTranspose2d of notebooks/05_more_image_inputs.ipynb
(csrc/conv2d_inputs_f32.hip, conv2d_functional, models/conv2d/nb05_more_inputs.py, data/nb05_datamodule.py) against float64 on
the CPU.

Tolerances are the project's own for exact-f32 conv kernels (conv2d_f32_helpers): ELEM_TOL per element relative to the
element's float64 sum of |products|, NORM_TOL relative norm for reductions.  The references are float64 F.conv2d and
torch.nn.grad.conv2d_weight.

The horizon ConvTranspose2d's shapes and its check (float64 autograd of the 33-channel F.conv_transpose2d) are
tests/conv_family_checks.py's, shared with its stride-2 twin of notebook 08.

The model-level checks (golden fixture, full size, determinism, HIP-graph replay, Trainer.fit) are notebook_model_checks.py's,
run by tests/test_gpu_notebook_models.py.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_family_checks as C
from conv2d_f32_helpers import NORM_TOL, ROOT, _ops, _rel, _within
from notebook_model_checks import _g, _randn

pytestmark = pytest.mark.gpu

# (batch, height, width) of the first layer's inputs: one output; odd sides; two column bands; full width; the model's size
INPUTS_SHAPES = [(1, 3, 3), (2, 4, 7), (3, 9, 70), (1, 5, 128), (2, 64, 64)]
PLANE_SCALES = (1.0, 0.25, 3.0, 7.0)        # flow prediction, t0 image, flow x, flow y: a swapped channel shows


# ---- the plain families' three passes: the records and the checker of tests/conv_family_checks.py ------------------------
@C.twin_shapes("convt2d_ae_horizon")
def test_horizon_conv_transpose_against_float64(device, twin, shape):
    C.check_horizon_conv_transpose(_ops(), device, twin, shape)


# ---- 1. Conv2d 4 -> 32 over three tensors read in place ------------------------------------------------------------------
@pytest.mark.parametrize("n, h, w", INPUTS_SHAPES)
def test_inputs_conv_against_float64(device, n, h, w):
    K = _ops()
    g = _g(500 + w + 3 * h)
    pred, t0 = _randn(g, n, h, w, scale=PLANE_SCALES[0]), _randn(g, n, h, w, scale=PLANE_SCALES[1])
    field = torch.stack((_randn(g, n, h, w, scale=PLANE_SCALES[2]), _randn(g, n, h, w, scale=PLANE_SCALES[3])), dim=1)
    wt, b = _randn(g, 32, 4, 3, 3, scale=36 ** -0.5), _randn(g, 32, scale=0.1)
    x64 = torch.cat((pred.unsqueeze(1), t0.unsqueeze(1), field), dim=1).double()
    w64, b64 = wt.double(), b.double()
    pre = F.conv2d(x64, w64, b64)
    absref = F.conv2d(x64.abs(), w64.abs(), b64.abs())
    assert tuple(pre.shape) == (n, 32, h - 2, w - 2)
    pd, td, fd, wd, bd = (t.to(device) for t in (pred, t0, field, wt, b))
    y = K.conv2d_ae_inputs_fwd_f32(pd, td, fd, wd, bd, relu=True)
    assert tuple(y.shape) == tuple(pre.shape)
    _within(y, pre.relu(), absref, what="forward relu")
    _within(K.conv2d_ae_inputs_fwd_f32(pd, td, fd, wd, bd, relu=False), pre, absref, what="forward without relu")
    _within(K.conv2d_ae_inputs_fwd_f32(pd, td, fd, wd, None, relu=False), pre - b64.view(1, -1, 1, 1), absref,
            what="forward plain")
    dy, dy_gate = _randn(g, *pre.shape), _randn(g, *pre.shape)
    for use_dg in (True, False):
        dyg = dy.double() * (dy_gate > 0) if use_dg else dy.double()
        dw, db = K.conv2d_ae_inputs_bwd_weight_f32(pd, td, fd, dy.to(device), tuple(wt.shape),
                                                   dy_gate=dy_gate.to(device) if use_dg else None)
        assert tuple(dw.shape) == (32, 4, 3, 3) and tuple(db.shape) == (32,)
        dw64 = torch.nn.grad.conv2d_weight(x64, tuple(wt.shape), dyg)
        for ch in range(4):      # each input plane on its own: a swapped or mis-strided channel shows at its own scale
            err = _rel(dw[:, ch], dw64[:, ch])
            assert err <= NORM_TOL, (use_dg, ch, err)
        assert _rel(db, dyg.sum((0, 2, 3))) <= NORM_TOL
        dw2, db2 = K.conv2d_ae_inputs_bwd_weight_f32(pd, td, fd, dy.to(device), tuple(wt.shape),
                                                     dy_gate=dy_gate.to(device) if use_dg else None)
        assert torch.equal(dw, dw2) and torch.equal(db, db2), "slab partials summed in slab order: identical bits"


# ---- 2. the data path on a hand-made device super-batch ------------------------------------------------------------------
def _hand_made_super_batch(device, t=5, h=40, w=36, border=6):
    """Pixel values encode (frame, row, column); the predictions carry a NaN border of 6 pixels; the field's x plane is the
    code + 0.25, its y plane the code + 0.5."""
    from predict_pv_yield_amd.data import flow_examples as fe
    rows, cols = torch.arange(h).view(1, h, 1).double(), torch.arange(w).view(1, 1, w).double()

    def code(frames, offset=0):
        return ((torch.arange(frames).view(-1, 1, 1) + offset) * 1e4 + rows * 1e2 + cols).float()

    index = torch.tensor([(t0, t0 + s) for t0 in range(t - 1) for s in range(1, t - t0)])
    preds = code(len(index), 100)
    for edge in (preds[:, :border], preds[:, -border:], preds[:, :, :border], preds[:, :, -border:]):
        edge.fill_(float("nan"))
    fields = torch.stack((code(t - 1, 200) + 0.25, code(t - 1, 200) + 0.5), dim=-1)
    return {fe.SAT_IMAGES: code(t).to(device), fe.OPTICAL_FLOW_FIELDS: fields.to(device),
            fe.OPTICAL_FLOW_PREDICTIONS: preds.to(device), fe.PREDICTION_INDEX: index}


def test_data_path_crops_one_window_from_all_four_tensors(device):
    from predict_pv_yield_amd.data import nb05_datamodule as D
    from predict_pv_yield_amd.data import flow_examples as fe
    sb = _hand_made_super_batch(device)
    s = 16
    rng = np.random.default_rng(7)
    examples = [D.super_batch_to_example(sb, rng, s) for _ in range(6)]
    index = sb[fe.PREDICTION_INDEX].numpy()
    for e in examples:
        assert e["input_images"].is_cuda and tuple(e["input_images"].shape) == (1, s, s)
        assert tuple(e["optical_flow"].shape) == (1, 2, s, s) and tuple(e["T0_IMAGES"].shape) == (1, s, s)
        assert e["forecast_horizon"].dtype == torch.float32 and e["forecast_horizon"].dim() == 0
        for k in ("input_images", "target_images", "T0_IMAGES", "optical_flow"):
            assert not torch.isnan(e[k]).any(), k
        first = float(e["input_images"][0, 0, 0])
        row, top, left = int(first // 1e4) - 100, int(first % 1e4 // 1e2), int(first % 1e2)
        assert 6 <= top <= 40 - 6 - s and 6 <= left <= 36 - 6 - s
        t0_idx, target_idx, flow_idx, horizon = D.pick_example_indices(index, 4, row)
        window = top * 1e2 + left
        # the four crops come from one window, each from the image the index rule names
        assert float(e["target_images"][0, 0, 0]) == target_idx * 1e4 + window
        assert float(e["T0_IMAGES"][0, 0, 0]) == t0_idx * 1e4 + window
        # planar, x before y, from the field at the target index clipped to the last field
        assert float(e["optical_flow"][0, 0, 0, 0]) == (200 + flow_idx) * 1e4 + window + 0.25
        assert float(e["optical_flow"][0, 1, 0, 0]) == (200 + flow_idx) * 1e4 + window + 0.5
        assert flow_idx == min(target_idx, 3)
        assert float(e["optical_flow"][0, 0, 1, 2]) == (200 + flow_idx) * 1e4 + window + 102.25      # rows, then columns
        assert float(e["input_images"][0, s - 1, s - 1]) == first + (s - 1) * 101
        assert float(e["forecast_horizon"]) == float(horizon)
    # equal seeds give equal examples
    rng = np.random.default_rng(7)
    for e in examples:
        twin = D.super_batch_to_example(sb, rng, s)
        assert all(torch.equal(e[k], twin[k]) for k in e)
    batch = fe.collate(examples)
    assert tuple(batch["optical_flow"].shape) == (6, 1, 2, s, s) and tuple(batch["forecast_horizon"].shape) == (6,)
    assert tuple(batch["input_images"].shape) == (6, 1, s, s) and batch["optical_flow"].is_contiguous()
    # a window that cannot avoid the NaN border: refused once the retries are spent, not silently kept
    with pytest.raises(D.ImageHasNansError):
        D.super_batch_to_example(sb, np.random.default_rng(1), 30, max_retries=4)


# ---- 3. one epoch through run.py's surface ---------------------------------------------------------------------------------
def test_one_epoch_of_the_configured_run(device, tmp_path, monkeypatch):
    """`run.py model=nb05_more_inputs datamodule=nb05_fake callbacks=none trainer.max_epochs=1` on a small fake set."""
    from predict_pv_yield_amd import hydra_lite as H
    from predict_pv_yield_amd.training import train
    from predict_pv_yield_amd.utils import extras
    monkeypatch.chdir(tmp_path)
    cfg = H.compose(os.path.join(ROOT, "configs"), "config",
                    ["model=nb05_more_inputs", "datamodule=nb05_fake", "callbacks=none", "trainer.max_epochs=1",
                     "trainer.gpus=1", "datamodule.batch_size=4", "datamodule.n_train_data=3", "datamodule.n_val_data=1",
                     "datamodule.n_super_batches=1", "datamodule.n_timesteps=6", "datamodule.frame_size_pixels=112",
                     "optimized_metric=Loss/Train_epoch"])
    extras(cfg)
    loss = train(cfg)
    assert np.isfinite(float(loss)), loss
