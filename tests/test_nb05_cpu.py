"""CPU: notebooks/05_more_image_inputs.ipynb's LitAutoEncoder.  tests/nb05_reference.py (float64, torch.nn.functional) is
pinned to the golden fixture, which the notebook's own cell produced (tests/golden/make_nb05_golden.py); then the model's names,
count and side rule, its refusals, the configs, the data path's host index rule against a literal restatement of the notebook's
arithmetic, and the C ABI's glue and refusals."""
import ctypes
import os

import numpy as np
import pytest
import torch

import nb05_reference as R
from conv2d_f32_helpers import NORM_TOL, ROOT, _rel
from notebook_model_checks import check_fit64
from test_conv2d_glue_cpu import T, check_glue_case, check_new_symbols

GOLDEN = os.path.join(ROOT, "tests", "golden", "nb05_small.npz")
NEW_SYMBOLS = {"pv_conv2d_ae_inputs_fwd_f32": 11, "pv_conv2d_ae_inputs_bwd_weight_workspace_bytes": 4,
               "pv_conv2d_ae_inputs_bwd_weight_f32": 13, "pv_convt2d_ae_horizon_fwd_f32": 10,
               "pv_convt2d_ae_horizon_bwd_weight_workspace_bytes": 4, "pv_convt2d_ae_horizon_bwd_weight_f32": 12}
N_PARAMS = 38753


@pytest.mark.parametrize("tag", ["a", "b"])
def test_reference_matches_the_golden(tag):
    gold = np.load(GOLDEN)
    batch, p = R.golden_case(gold, tag)
    p = R.params64(p)
    y_hat = R.forward64(p, batch)
    c = R.G.CASES[tag]
    assert tuple(y_hat.shape) == tuple(gold[f"{tag}/y_hat"].shape) == (len(c["minutes"]), 1, c["h"], c["w"])
    assert _rel(y_hat.detach(), gold[f"{tag}/y_hat"]) <= 1e-5
    loss = R.loss64(y_hat, batch["target_images"])
    assert abs(loss.item() - gold[f"{tag}/losses"][0]) <= 1e-5 * gold[f"{tag}/losses"][0]
    loss.backward()
    for k, v in p.items():
        assert _rel(v.grad, gold[f"{tag}/grad/{k}"]) <= NORM_TOL, k
    check_fit64(R, gold, tag, batch, "target_images")


def test_golden_cases_are_the_ones_the_issue_names():
    a, b = R.G.draw_batch("a"), R.G.draw_batch("b")
    for batch, (n, h, w) in ((a, (3, 16, 16)), (b, (2, 12, 20))):
        for key in ("input_images", "T0_IMAGES", "target_images"):
            assert tuple(batch[key].shape) == (n, 1, h, w)
        assert tuple(batch["optical_flow"].shape) == (n, 1, 2, h, w)
    want = [(np.float32(m) - np.float32(62.5)) / np.float32(34.61) for m in (5, 45, 115)]
    assert a["forecast_horizon"].tolist() == [float(v) for v in want] and a["forecast_horizon"].dtype == torch.float32
    gold = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 1 << 20
    assert sorted(k.split("/")[1] for k in gold.files if k.startswith("a/")) == sorted(
        ["y_hat", "losses"] + ["grad"] * 12 + ["step3"] * 12)        # results only


def test_names_shapes_count_and_side_rule():
    from predict_pv_yield_amd.models.conv2d import nb05_more_inputs as M
    assert [M.output_side(s) for s in (7, 64, 128)] == [7, 64, 128]
    assert M.MIN_IMAGE_SIDE == 7 and M.MAX_IMAGE_SIDE == 128 and (M.STRIDE, M.GROUPS, M.CHANNELS) == (1, 1, 32)
    for side in (6, 129, 0):
        with pytest.raises(ValueError, match="7 to 128"):
            M.output_side(side)
    M.check_target_side((64, 64), (7, 1, 64, 64))
    M.check_target_side((12, 20), (2, 1, 12, 20))
    for bad in ((7, 1, 62, 64), (7, 64, 64), (7, 2, 64, 64)):
        with pytest.raises(ValueError, match="target_images"):
            M.check_target_side((64, 64), bad)
    model = M.LitAutoEncoder()
    assert sum(p.numel() for p in model.parameters()) == N_PARAMS
    assert list(model.state_dict()) == [f"{part}.{i}.{w}" for part in ("encoder", "decoder") for i in (0, 2, 4)
                                        for w in ("weight", "bias")]
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == R.G.PARAM_SHAPES
    # the sides of the two nn.Sequential the model holds, on the CPU: S -> S - 6 -> S
    for h, w in ((7, 7), (12, 20), (64, 64)):
        enc = model.encoder(torch.zeros(1, 4, h, w))
        assert tuple(enc.shape) == (1, 32, h - 6, w - 6)
        dec = model.decoder(torch.cat((enc, torch.zeros(1, 1, *enc.shape[2:])), dim=1))
        assert tuple(dec.shape) == (1, 1, M.output_side(h), M.output_side(w))
    opt = model.configure_optimizers()
    assert type(opt).__name__ == "HipAdam" and opt.param_groups[0]["lr"] == 1e-3
    assert M.LitAutoEncoder(lr=1e-4).configure_optimizers().param_groups[0]["lr"] == 1e-4
    # the scaffold's keys: this model names its own, the others keep theirs
    from predict_pv_yield_amd.models._notebook_ae import NotebookAutoEncoder
    assert (M.LitAutoEncoder.image_key, M.LitAutoEncoder.target_key) == ("input_images", "target_images")
    assert (NotebookAutoEncoder.image_key, NotebookAutoEncoder.target_key) == ("HISTORICAL_SAT_IMAGES", "TARGET_SAT_IMAGE")


def test_model_refusals_on_the_cpu():
    from predict_pv_yield_amd.models.conv2d import nb05_more_inputs as M
    z = torch.zeros
    model = M.LitAutoEncoder()
    batch = {"input_images": z(2, 1, 16, 16), "T0_IMAGES": z(2, 1, 16, 16), "optical_flow": z(2, 1, 2, 16, 16),
             "forecast_horizon": torch.tensor([0.1, -0.2]), "target_images": z(2, 1, 16, 16)}
    with pytest.raises(RuntimeError, match="MI355X only"):
        model(batch)
    with pytest.raises(RuntimeError, match="MI355X only"):
        model({**batch, "optical_flow": z(2, 2, 16, 16)})          # the planar field without its singleton axis is accepted
    with pytest.raises(ValueError, match="target_images"):
        model.training_step({**batch, "target_images": z(2, 1, 14, 14)}, 0)
    with pytest.raises(ValueError, match="target_images"):
        model.training_step({**batch, "target_images": z(2, 16, 16)}, 0)
    for side in (6, 129):
        sized = {k: z(2, 1, side, side) for k in ("input_images", "T0_IMAGES", "target_images")}
        with pytest.raises(ValueError, match="7 to 128"):
            model.training_step({**batch, **sized, "optical_flow": z(2, 1, 2, side, side)}, 0)
    # refused before the device is looked at: no channel axis, two channels, a t0 image of another size
    for pred in (z(2, 16, 16), z(2, 2, 16, 16)):
        with pytest.raises(ValueError, match="input_images"):
            model({**batch, "input_images": pred})
    with pytest.raises(ValueError, match="T0_IMAGES"):
        model({**batch, "T0_IMAGES": z(2, 1, 16, 15)})
    # a field that is interleaved, of three planes, of another size or of another batch
    for field in (z(2, 16, 16, 2), z(2, 1, 3, 16, 16), z(2, 1, 2, 16, 15), z(3, 1, 2, 16, 16), z(2, 1, 1, 2, 16, 16)):
        with pytest.raises(ValueError, match="optical_flow"):
            model({**batch, "optical_flow": field})
    with pytest.raises(ValueError, match="forecast_horizon"):
        model({**batch, "forecast_horizon": z(3)})


def test_host_index_rule_against_the_notebooks_arithmetic():
    """pick_example_indices against super_batch_to_example's statements, written out: the horizon as float32 minutes, -= 62.5,
    /= 34.61; target_idx.clip(max=n_optical_flows - 1) -- the field at the *target* index, clipped at the last field."""
    from predict_pv_yield_amd.data import nb05_datamodule as D
    n_images = 6
    n_flows = n_images - 1
    index = np.array([(t0, t0 + s) for t0 in range(n_flows) for s in range(1, n_flows - t0 + 1)])       # (t0, target)
    assert len(index) == n_flows * n_images // 2
    for row, (t0, target) in enumerate(index):
        horizon = np.timedelta64(int(target - t0) * 5, "m").astype(np.float32)
        horizon -= 62.5
        horizon /= 34.61
        want_flow = np.int64(target).clip(max=n_flows - 1)
        got = D.pick_example_indices(index, n_flows, row)
        assert got[:3] == (t0, target, int(want_flow))
        assert got[3] == np.float32(horizon) and isinstance(got[3], np.float32)
    # the last image has no field of its own: clipped
    assert D.pick_example_indices(index, n_flows, n_flows - 1)[:3] == (0, 5, 4)
    assert D.pick_example_indices(index, n_flows, 0)[:3] == (0, 1, 1)
    # subtract, then divide, each rounded to float32 (115 minutes: the one-step form differs from float64's by an ulp or none)
    for m in (5, 45, 115, 120):
        assert D.normalise_forecast_horizon(m) == np.float32(np.float32(np.float32(m) - np.float32(62.5)) / np.float32(34.61))
    # the prediction row is uniform over all P: one draw, rng.integers(0, P)
    rng, twin = np.random.default_rng(3), np.random.default_rng(3)
    for _ in range(8):
        row = int(twin.integers(low=0, high=len(index)))
        assert D.draw_example_indices(rng, index, n_flows) == (row, *D.pick_example_indices(index, n_flows, row))


def test_sample_squares_on_the_cpu_follows_the_notebooks_draws():
    """One (top, left) for all four tensors, top drawn before left with rng.integers(0, max); a square with a NaN is drawn
    again; the field's crop is planar, x before y; ImageHasNansError once the retries are spent."""
    from predict_pv_yield_amd.data import nb05_datamodule as D
    h, w, s = 20, 17, 8
    rows, cols = torch.arange(h).view(h, 1).float(), torch.arange(w).view(1, w).float()
    code = rows * 100 + cols
    pred = code.clone()
    pred[:3], pred[:, :2] = float("nan"), float("nan")
    example = {"input_images": pred[None], "target_images": (code + 1e4)[None], "T0_IMAGES": (code + 2e4)[None],
               "optical_flow": torch.stack((code + 3e4, code + 4e4), dim=-1)[None], "forecast_horizon": torch.tensor(0.5)}
    rng, twin = np.random.default_rng(11), np.random.default_rng(11)
    for _ in range(6):
        out = D.sample_squares(example, rng, s)
        while True:
            top = int(twin.integers(low=0, high=h - s))
            left = int(twin.integers(low=0, high=w - s))
            if top >= 3 and left >= 2:
                break
        base = top * 100 + left
        assert out["input_images"][0, 0, 0] == base and out["target_images"][0, 0, 0] == base + 1e4
        assert out["T0_IMAGES"][0, 0, 0] == base + 2e4
        assert tuple(out["optical_flow"].shape) == (1, 2, s, s)
        assert out["optical_flow"][0, 0, 0, 0] == base + 3e4 and out["optical_flow"][0, 1, 0, 0] == base + 4e4
        assert out["optical_flow"][0, 0, 1, 0] == base + 3e4 + 100           # rows stay rows
        assert not any(torch.isnan(out[k]).any() for k in ("input_images", "target_images", "T0_IMAGES", "optical_flow"))
        assert out["forecast_horizon"] == 0.5
    with pytest.raises(D.ImageHasNansError, match="3 retries"):
        D.sample_squares({**example, "T0_IMAGES": torch.full((1, h, w), float("nan"))}, rng, s, max_retries=3)


def test_glue_refuses_bad_shapes_before_touching_a_device():
    from predict_pv_yield_amd import hip_ops as K
    z = torch.zeros
    w4, b32 = z(32, 4, 3, 3), z(32)
    with pytest.raises(ValueError, match="t0 image"):
        K.conv2d_ae_inputs_fwd_f32(z(2, 8, 8), z(2, 8, 9), z(2, 2, 8, 8), w4, b32)
    with pytest.raises(ValueError, match="t0 image"):
        K.conv2d_ae_inputs_fwd_f32(z(2, 1, 8, 8), z(2, 1, 8, 8), z(2, 2, 8, 8), w4, b32)
    with pytest.raises(ValueError, match="flow field"):
        K.conv2d_ae_inputs_fwd_f32(z(2, 8, 8), z(2, 8, 8), z(2, 8, 8, 2), w4, b32)
    with pytest.raises(ValueError, match="weight"):
        K.conv2d_ae_inputs_fwd_f32(z(2, 8, 8), z(2, 8, 8), z(2, 2, 8, 8), z(16, 4, 3, 3), z(16))
    with pytest.raises(ValueError, match="weight"):
        K.conv2d_ae_inputs_bwd_weight_f32(z(2, 8, 8), z(2, 8, 8), z(2, 2, 8, 8), z(2, 32, 6, 6), (32, 6, 3, 3))
    with pytest.raises(ValueError, match="x \\[N, 32"):
        K.convt2d_ae_horizon_fwd_f32(z(2, 33, 4, 4), z(2), z(33, 32, 3, 3), z(32))
    with pytest.raises(ValueError, match="weight"):
        K.convt2d_ae_horizon_fwd_f32(z(2, 32, 4, 4), z(2), z(32, 32, 3, 3), z(32))
    with pytest.raises(ValueError, match="horizon"):
        K.convt2d_ae_horizon_fwd_f32(z(2, 32, 4, 4), z(3), z(33, 32, 3, 3), z(32))
    with pytest.raises(ValueError, match="128 columns"):
        K.convt2d_ae_horizon_fwd_f32(z(2, 32, 4, 127), z(2), z(33, 32, 3, 3), z(32))
    with pytest.raises(ValueError, match="bias"):
        K.convt2d_ae_horizon_fwd_f32(z(2, 32, 4, 4), z(2), z(33, 32, 3, 3), z(33))
    with pytest.raises(ValueError, match="dy"):
        K.convt2d_ae_horizon_bwd_weight_f32(z(2, 32, 4, 4), z(2), z(2, 32, 9, 9), None, (33, 32, 3, 3))


def test_config_composes_and_instantiates():
    from predict_pv_yield_amd import hydra_lite as H
    cfg = H.compose(os.path.join(ROOT, "configs"), "config", ["model=nb05_more_inputs", "datamodule=nb05_fake",
                                                              "callbacks=none", "trainer.max_epochs=1"])
    assert cfg.model._target_ == "predict_pv_yield_amd.models.conv2d.nb05_more_inputs.LitAutoEncoder"
    assert cfg.datamodule._target_ == "predict_pv_yield_amd.data.nb05_datamodule.Nb05DataModule"
    model, dm = H.instantiate(cfg.model), H.instantiate(cfg.datamodule)
    assert sum(p.numel() for p in model.parameters()) == N_PARAMS and dm.batch_size == 64 and dm.image_size_pixels == 64
    assert model.configure_optimizers().param_groups[0]["lr"] == 1e-3


def test_new_symbols_are_declared_and_bound_with_matching_arity():
    check_new_symbols(NEW_SYMBOLS, "05_more_image_inputs.ipynb")


def test_entry_points_refuse_bad_arguments_without_launching():
    """A plane under 3 or over 128 wide, a tensor beyond 32-bit indexing, a null pointer, a non-positive size, a short
    workspace: the ABI's error code and a message, from pointers that are never dereferenced."""
    from predict_pv_yield_amd import _lib
    lib = _lib.get_lib()
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    need = ctypes.c_size_t(0)
    ESIZE, EINVAL = -2, -1

    def err():
        return lib.pv_last_error().decode()

    # the four-input first layer: (flow_pred, t0, flow_field, w, bias, y, n, h, w_img, relu, stream)
    assert lib.pv_conv2d_ae_inputs_fwd_f32(p, p, p, p, p, p, 2, 2, 20, 1, None) == ESIZE and "kernel" in err()
    assert lib.pv_conv2d_ae_inputs_fwd_f32(p, p, p, p, p, p, 2, 20, 2, 1, None) == ESIZE and "kernel" in err()
    assert lib.pv_conv2d_ae_inputs_fwd_f32(p, p, p, p, p, p, 2, 20, 129, 1, None) == ESIZE and "128" in err()
    assert lib.pv_conv2d_ae_inputs_fwd_f32(p, p, p, p, p, p, 1 << 13, 128, 128, 1, None) == ESIZE and "2^31" in err()
    assert lib.pv_conv2d_ae_inputs_fwd_f32(p, p, p, p, p, p, 0, 20, 20, 1, None) == EINVAL
    for null_at in (0, 1, 2, 3, 5):
        args = [p] * 6
        args[null_at] = None
        assert lib.pv_conv2d_ae_inputs_fwd_f32(*args, 2, 20, 20, 1, None) == EINVAL and "null" in err()
    assert lib.pv_conv2d_ae_inputs_fwd_f32(p, p, p, p, None, p, 2, 20, 129, 1, None) == ESIZE      # a null bias is allowed
    assert lib.pv_conv2d_ae_inputs_bwd_weight_workspace_bytes(2, 20, 129, ctypes.byref(need)) == ESIZE
    assert lib.pv_conv2d_ae_inputs_bwd_weight_workspace_bytes(2, 2, 20, ctypes.byref(need)) == ESIZE
    assert lib.pv_conv2d_ae_inputs_bwd_weight_workspace_bytes(-1, 20, 20, ctypes.byref(need)) == EINVAL
    assert lib.pv_conv2d_ae_inputs_bwd_weight_workspace_bytes(2, 20, 20, None) == EINVAL
    assert lib.pv_conv2d_ae_inputs_bwd_weight_workspace_bytes(2, 20, 20, ctypes.byref(need)) == 0 and need.value > 0
    assert lib.pv_conv2d_ae_inputs_bwd_weight_f32(p, p, p, p, None, p, p, 2, 20, 20, p, need.value - 1, None) == EINVAL
    assert "workspace" in err()
    assert lib.pv_conv2d_ae_inputs_bwd_weight_f32(p, p, p, p, None, p, p, 2, 20, 20, None, need.value, None) == EINVAL
    assert lib.pv_conv2d_ae_inputs_bwd_weight_f32(p, p, p, None, None, p, p, 2, 20, 20, p, need.value, None) == EINVAL
    assert lib.pv_conv2d_ae_inputs_bwd_weight_f32(p, p, p, p, None, p, p, 2, 20, 129, p, 1 << 30, None) == ESIZE
    # the horizon ConvTranspose2d at stride 1: (x, horizon, w, bias, y, n, h_in, w_in, relu, stream)
    assert lib.pv_convt2d_ae_horizon_fwd_f32(p, p, p, p, p, 2, 15, 127, 1, None) == ESIZE and "width" in err()
    assert lib.pv_convt2d_ae_horizon_fwd_f32(p, p, p, p, p, 2, 0, 15, 1, None) == EINVAL
    assert lib.pv_convt2d_ae_horizon_fwd_f32(p, p, p, p, p, 0, 15, 15, 1, None) == EINVAL
    assert lib.pv_convt2d_ae_horizon_fwd_f32(p, None, p, p, p, 2, 15, 15, 1, None) == EINVAL and "null" in err()
    assert lib.pv_convt2d_ae_horizon_fwd_f32(p, p, p, p, p, 1 << 20, 63, 63, 1, None) == ESIZE and "2^31" in err()
    assert lib.pv_convt2d_ae_horizon_fwd_f32(p, p, p, None, p, 2, 15, 127, 1, None) == ESIZE       # a null bias is allowed
    assert lib.pv_convt2d_ae_horizon_bwd_weight_workspace_bytes(2, 15, 127, ctypes.byref(need)) == ESIZE
    assert lib.pv_convt2d_ae_horizon_bwd_weight_workspace_bytes(2, 15, 15, None) == EINVAL
    assert lib.pv_convt2d_ae_horizon_bwd_weight_workspace_bytes(2, 15, 15, ctypes.byref(need)) == 0 and need.value > 0
    assert lib.pv_convt2d_ae_horizon_bwd_weight_f32(p, p, p, None, p, p, 2, 15, 15, p, need.value - 1, None) == EINVAL
    assert "workspace" in err()
    assert lib.pv_convt2d_ae_horizon_bwd_weight_f32(p, p, None, None, p, p, 2, 15, 15, p, need.value, None) == EINVAL
    assert lib.pv_convt2d_ae_horizon_bwd_weight_f32(p, p, p, None, p, p, 2, 15, 127, p, 1 << 30, None) == ESIZE


# ---- what the new wrappers hand to the C ABI (the harness of tests/test_conv2d_glue_cpu.py) --------------------------------
INPUTS = dict(flow_pred=T(2, 9, 11), t0=T(2, 9, 11), flow_field=T(2, 2, 9, 11))
GLUE = {
    "inputs_fwd": (
        "conv2d_ae_inputs_fwd_f32", dict(**INPUTS, weight=T(32, 4, 3, 3), bias=T(32), relu=True),
        ["require_cuda", "require_cuda", "pv_conv2d_ae_inputs_fwd_f32 flow_pred t0 flow_field weight bias out0 2 9 11 1 stream"],
        ["(2, 32, 7, 9) float32"], []),
    "inputs_fwd/none": (
        "conv2d_ae_inputs_fwd_f32", dict(**INPUTS, weight=T(32, 4, 3, 3), bias=None, relu=False),
        ["require_cuda", "require_cuda", "pv_conv2d_ae_inputs_fwd_f32 flow_pred t0 flow_field weight NULL out0 2 9 11 0 stream"],
        ["(2, 32, 7, 9) float32"], []),
    "inputs_bwd_weight": (
        "conv2d_ae_inputs_bwd_weight_f32", dict(**INPUTS, dy=T(2, 32, 7, 9), weight_shape=(32, 4, 3, 3), dy_gate=T(2, 32, 7, 9)),
        ["require_cuda", "require_cuda", "pv_conv2d_ae_inputs_bwd_weight_workspace_bytes 2 9 11 &bytes",
         "pv_conv2d_ae_inputs_bwd_weight_f32 flow_pred t0 flow_field dy dy_gate out0 out1 2 9 11 ws:conv2d_ae_inputs_wgrad 4096 "
         "stream"],
        ["(32, 4, 3, 3) float32", "(32,) float32"], ["conv2d_ae_inputs_wgrad"]),
    "horizon_fwd": (
        "convt2d_ae_horizon_fwd_f32", dict(x=T(2, 32, 4, 5), horizon=T(2), weight=T(33, 32, 3, 3), bias=T(32), relu=True),
        ["require_cuda", "pv_convt2d_ae_horizon_fwd_f32 x horizon weight bias out0 2 4 5 1 stream"],
        ["(2, 32, 6, 7) float32"], []),
    "horizon_bwd_weight": (
        "convt2d_ae_horizon_bwd_weight_f32", dict(x=T(2, 32, 4, 5), horizon=T(2), dy=T(2, 32, 6, 7), dy_gate=None,
                                                  weight_shape=(33, 32, 3, 3)),
        ["require_cuda", "pv_convt2d_ae_horizon_bwd_weight_workspace_bytes 2 4 5 &bytes",
         "pv_convt2d_ae_horizon_bwd_weight_f32 x horizon dy NULL out0 out1 2 4 5 ws:convt2d_ae_horizon_wgrad 4096 stream"],
        ["(33, 32, 3, 3) float32", "(32,) float32"], ["convt2d_ae_horizon_wgrad"]),
}


@pytest.mark.parametrize("case_id", sorted(GLUE))
def test_new_wrappers_hand_the_abi_what_the_table_pins(monkeypatch, case_id):
    check_glue_case(monkeypatch, GLUE[case_id])


def test_functional_names_the_new_layers_and_chain():
    from predict_pv_yield_amd import conv2d_functional as C
    from predict_pv_yield_amd import hip_ops as K
    assert C.INPUTS_AE_OPS == (K.conv2d_ae_inputs_fwd_f32, K.conv2d_ae_inputs_bwd_weight_f32)
    assert callable(C.nb05_more_inputs_f32) and issubclass(C.HorizonConvTransposeS1ReLU, torch.autograd.Function)
