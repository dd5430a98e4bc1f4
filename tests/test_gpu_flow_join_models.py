"""GPU: the optical-flow join of the six satellite models that read frames past t0 (the reference's
`# TODO: Use optical flow, not actual sat images of the future!`): the two kernels it adds (u8 stacks straight from normalised
f32 input of either layout; cv.remap on channels-last frames), `replace_future_frames_with_flow(layout=, flow_channel=)`
and the models' `future_frames` / `flow_channel` knobs.

Inputs are data.synthetic.advected_counts (the dense blob texture) normalised on the host with SAT_MEAN / SAT_STD: on flat
inputs Farnebäck's regulariser returns zero flow and every check below would be vacuous.
"""
import os

import numpy as np
import pytest
import torch

from oracle import flow_oracle as fo
from predict_pv_yield_amd.data.synthetic import advected_counts
from tests.test_gpu_flow import _random_flow, same_f32

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS_SCALE = 255.0 / 6.0          # the default of replace_future_frames_with_flow


def _of():
    from predict_pv_yield_amd import optical_flow
    return optical_flow


def _ops():
    from predict_pv_yield_amd import hip_ops
    return hip_ops


def _mean_std(c):
    of = _of()
    return (of.SAT_MEAN[:c], of.SAT_STD[:c]) if c == 12 else (of.SAT_MEAN[1:1 + c], of.SAT_STD[1:1 + c])


def _normalised(b, t, c, h, w, seed):
    """advected_counts normalised on the host -> planar f32 [B, C, T, H, W] (NumPy) and the per-channel std."""
    raw, _ = advected_counts(batch=b, t=t, channels=c, h=h, w=w, seed=seed)
    mean, std = _mean_std(c)
    x = (raw.astype(np.float32) - mean[None, None, :, None, None]) / std[None, None, :, None, None]
    return np.ascontiguousarray(x.transpose(0, 2, 1, 3, 4)).astype(np.float32), std


def _u8_reference(x, s):
    """flow_oracle.convert_10bpp_to_uint8(clip(float32(x * s) + 512, 0, 1020), 0) in NumPy float32."""
    counts = np.clip((x * s).astype(np.float32) + np.float32(512.0), np.float32(0.0), np.float32(1020.0)).astype(np.float32)
    return fo.convert_10bpp_to_uint8(counts, 0)[0]


# ---- 1. K1 alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,t,c,h,w", [(2, 7, 12, 32, 32), (1, 3, 5, 37, 50), (2, 13, 12, 64, 64)])
@pytest.mark.parametrize("layout", ["NCTHW", "NTHWC"])
def test_u8_stacks_from_normalised_bit_exact(device, b, t, c, h, w, layout):
    K = _ops()
    rng = np.random.default_rng(b * 1000 + t * 100 + c)
    s = np.float32(4.0 * COUNTS_SCALE)
    mean, std = _mean_std(12)
    raw, _ = advected_counts(batch=b, t=t, channels=c, h=h, w=w, seed=31 + c)
    x = ((raw.astype(np.float32) - mean[None, None, :c, None, None]) / std[None, None, :c, None, None]).astype(np.float32)
    x = np.ascontiguousarray(x.transpose(0, 2, 1, 3, 4))                    # [B, C, T, H, W]
    # values that clamp at both ends, the ends themselves, and exact rounding ties: x * s + 512 = 4 k + 2 in f32 (the product
    # lies within 2^-15 of the even integer 4 k + 2 - 512, so the sum is that integer: 512..1024 has a spacing of 2^-14)
    flat = x.reshape(-1)
    special = [-20.0, -3.5, 3.5, 20.0, -512.0 / float(s), 508.0 / float(s), 0.0]
    special += [float(np.float32((4 * k + 2 - 512) / float(s))) for k in (0, 1, 2, 63, 127, 128, 129, 200, 253, 254)]
    pos = rng.choice(flat.size, size=len(special) * 8, replace=False)
    flat[pos] = np.tile(np.asarray(special, np.float32), 8)
    ties = (x * s).astype(np.float32) + np.float32(512.0)
    assert np.sum((ties % 4 == 2) & (ties > 0) & (ties < 1020)) >= 10, "the tie constructions must be ties"
    assert (ties < 0).any() and (ties > 1020).any()
    t_obs = max(2, t - 2)
    ref = _u8_reference(x[:, :, :t_obs], s)                                 # [B, C, t_obs, H, W]
    xt = torch.from_numpy(x).to(device)
    if layout == "NTHWC":
        xt = xt.permute(0, 2, 3, 4, 1).contiguous()
    before = xt.clone()
    got = K.u8_stacks_from_normalised(xt, t_obs, COUNTS_SCALE, layout)
    assert got.shape == (b, c, t_obs, h, w) and got.dtype == torch.uint8
    assert np.array_equal(got.cpu().numpy(), ref)
    for ch in sorted({0, c // 2, c - 1}):
        one = K.u8_stacks_from_normalised(xt, t_obs, COUNTS_SCALE, layout, channel=ch)
        assert one.shape == (b, 1, t_obs, h, w)
        assert np.array_equal(one.cpu().numpy()[:, 0], ref[:, ch]), ch
    assert torch.equal(xt, before)


def test_u8_stacks_take_strided_views_and_refuse_bad_arguments(device):
    K = _ops()
    x, _ = _normalised(2, 6, 4, 16, 24, seed=5)
    s = np.float32(4.0 * COUNTS_SCALE)
    big = torch.from_numpy(x).to(device)
    view = big[:, 1:4, 1:]                                                  # channel and time offsets: not contiguous
    got = K.u8_stacks_from_normalised(view, 3, COUNTS_SCALE, "NCTHW")
    assert np.array_equal(got.cpu().numpy(), _u8_reference(x[:, 1:4, 1:4], s))
    with pytest.raises(ValueError):
        K.u8_stacks_from_normalised(big, 3, COUNTS_SCALE, "NHWC")
    with pytest.raises(ValueError):
        K.u8_stacks_from_normalised(big, 7, COUNTS_SCALE)
    with pytest.raises(ValueError):
        K.u8_stacks_from_normalised(big, 3, COUNTS_SCALE, channel=4)
    with pytest.raises(TypeError):
        K.u8_stacks_from_normalised(big.double(), 3, COUNTS_SCALE)
    with pytest.raises(TypeError):
        K.u8_stacks_from_normalised(big[:, :, :, ::2], 3, COUNTS_SCALE)    # every other row: one pixel stride cannot say that


# ---- 2. K2 alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(32, 32), (64, 64), (37, 50)])
@pytest.mark.parametrize("c", [1, 5, 12])
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("border", [fo.BORDER_CONSTANT, fo.BORDER_REPLICATE])
def test_remap_nhwc_bit_exact(device, h, w, c, shared, border):
    K = _ops()
    rng = np.random.default_rng(h * w + 7 * c + border + 100 * shared)
    n, n_steps = 3, 4
    imgs = rng.normal(0, 1, (n, h, w, c)).astype(np.float32)
    nf = 1 if shared else c
    flows = np.stack([np.stack([_random_flow(rng, h, w, 2.5) for _ in range(nf)]) for _ in range(n)])   # [n, nf, h, w, 2]
    # the constructions of tests/test_gpu_flow.py::test_remap_f32_bit_exact (and of its LDS variant), per image
    flows[0] = np.round(flows[0] * 32) / 32           # exact 1/32 fractions
    flows[1, :, :4] = np.round(flows[1, :, :4])       # integer shifts
    flows[2, :, 0, 0] = [np.nan, 1e12]                # NaN / overflow coordinates
    flows[2, :, 1, 1] = [0.015625, -0.046875]         # cvRound ties (x.5/32)
    flows[2, -1, 8:] *= 20.0                          # mostly outside the image
    # frames one time slice apart inside a [N, T, H, W, C] tensor, as the join calls it
    t = n_steps + 2
    stack = torch.full((n, t, h, w, c), 7.0, dtype=torch.float32, device=device)
    stack[:, 1] = torch.from_numpy(imgs).to(device)
    fl = torch.from_numpy(np.ascontiguousarray(flows[:, 0]) if shared else flows).to(device)
    K.remap_bilinear_nhwc(stack[:, 1], fl, stack[:, 2:], 1.0, border, float("nan"))
    got = stack.cpu().numpy()
    assert np.array_equal(got[:, 1], imgs) and np.all(got[:, 0] == 7.0)
    for i in range(n):
        for ch in range(c):
            for s in range(n_steps):
                ref = fo.remap_image(np.ascontiguousarray(imgs[i, :, :, ch]), flows[i, 0 if shared else ch], float(1 + s),
                                     border, np.nan)
                assert same_f32(got[i, 2 + s, :, :, ch], ref), (i, ch, s)


def test_remap_nhwc_refuses_bad_arguments(device):
    K = _ops()
    src = torch.zeros(2, 8, 8, 4, device=device)
    out = torch.zeros(2, 3, 8, 8, 4, device=device)
    with pytest.raises(TypeError):
        K.remap_bilinear_nhwc(src, torch.zeros(2, 8, 8, 3, device=device), out)
    with pytest.raises(TypeError):
        K.remap_bilinear_nhwc(src, torch.zeros(2, 4, 8, 8, 2, device=device), out[..., :3])
    with pytest.raises(TypeError):
        K.remap_bilinear_nhwc(src.permute(0, 2, 1, 3), torch.zeros(2, 8, 8, 2, device=device), out)


# ---- 3. / 4. the public function: layouts agree, defaults keep their bits --------------------------------------------------
@pytest.mark.parametrize("flow_channel", [None, 0])
@pytest.mark.parametrize("b,c,h,w", [(2, 12, 32, 32), (3, 2, 37, 50)])
def test_layouts_agree_bit_for_bit(device, flow_channel, b, c, h, w):
    of = _of()
    x, _ = _normalised(b, 7, c, h, w, seed=77)
    n_future = 5
    x = np.concatenate([x, np.full((b, c, n_future, h, w), np.nan, np.float32)], axis=2)   # the true future is never read
    planar = torch.from_numpy(x).to(device)
    last = planar.permute(0, 2, 3, 4, 1).contiguous()
    a = of.replace_future_frames_with_flow(planar, n_future, flow_channel=flow_channel)
    z = of.replace_future_frames_with_flow(last, n_future, layout="NTHWC", flow_channel=flow_channel)
    assert a.shape == planar.shape and z.shape == last.shape and z.is_contiguous()
    assert torch.isfinite(a).all()
    assert torch.equal(z.permute(0, 4, 1, 2, 3), a)


def test_shared_flow_is_channel_0s_flow_and_differs_from_per_channel(device):
    of = _of()
    x, _ = _normalised(2, 9, 4, 32, 32, seed=3)
    planar = torch.from_numpy(x).to(device)
    own = of.replace_future_frames_with_flow(planar, 3)
    shared = of.replace_future_frames_with_flow(planar, 3, flow_channel=0)
    assert torch.equal(own[:, 0], shared[:, 0])                 # channel 0 along its own flow either way
    assert not torch.equal(own[:, 1:], shared[:, 1:])           # each texture moves with its own velocity
    two = of.replace_future_frames_with_flow(planar, 3, flow_channel=2)
    assert torch.equal(own[:, 2], two[:, 2])
    # one sample (its channels along the one field, flow stride 0) is the same arithmetic as a batch of them
    assert torch.equal(of.replace_future_frames_with_flow(planar[:1], 3, flow_channel=0), shared[:1])
    assert torch.equal(of.replace_future_frames_with_flow(planar[:, :1].contiguous(), 3, flow_channel=0), shared[:, :1])


@pytest.mark.parametrize("b,c,t,h,w,n_future", [(2, 11, 12, 64, 64, 6), (2, 12, 10, 24, 24, 4), (1, 3, 6, 37, 50, 2)])
def test_defaults_keep_their_bits(device, b, c, t, h, w, n_future):
    """Default arguments on a planar input: the bits of the chain the function was before (torch multiply, add, clamp, then
    u8_from_10bit, farneback_stack, flow_weighted_mean, remap_bilinear), spelled out from the hip_ops primitives."""
    of, K = _of(), _ops()
    x, _ = _normalised(b, t, c, h, w, seed=11)
    sat = torch.from_numpy(x).to(device)
    before = sat.clone()
    t_obs = t - n_future
    obs = sat[:, :, :t_obs].contiguous()
    counts = ((obs * (4.0 * COUNTS_SCALE)) + 512.0).clamp_(0.0, 1020.0)
    u8 = K.u8_from_10bit(counts, 0)
    flows = K.farneback_stack(u8, **of.REFERENCE_FARNEBACK_KWARGS)
    mean_flow = K.flow_weighted_mean(flows.view(b * c, t_obs - 1, h, w, 2))
    adv = K.remap_bilinear(obs[:, :, -1].contiguous().view(b * c, h, w), mean_flow, n_steps=n_future, step0=1.0,
                           border_mode=of.BORDER_REPLICATE, border_value=float("nan"))
    old = torch.cat([obs, adv.view(b, c, n_future, h, w)], dim=2)
    new = of.replace_future_frames_with_flow(sat, n_future)
    assert new.is_contiguous() and new.data_ptr() != sat.data_ptr()
    assert torch.equal(new, old)
    assert torch.equal(sat, before)                              # the input is not written
    assert float((new[:, :, t_obs:] - sat[:, :, t_obs:]).abs().max()) > 0     # and the future slices were replaced


def test_replace_future_frames_refuses_bad_arguments(device):
    of = _of()
    sat = torch.zeros(1, 2, 6, 16, 16, device=device)
    with pytest.raises(ValueError, match="layout"):
        of.replace_future_frames_with_flow(sat, 2, layout="NHWC")
    with pytest.raises(ValueError, match="flow_channel"):
        of.replace_future_frames_with_flow(sat, 2, flow_channel=2)
    with pytest.raises(ValueError, match="two observed"):
        of.replace_future_frames_with_flow(sat, 5)
    with pytest.raises(TypeError):
        of.replace_future_frames_with_flow(sat.half(), 2)


# ---- 5. against the oracle chain ------------------------------------------------------------------------------------------
def _check(what, value, bound):
    print(f"[flow-join] {what}: {value:.3e} (bound {bound:.1e})")
    assert value <= bound, f"{what}: {value} > {bound}"


def _oracle_chain(x_obs, n_future, flow_channel):
    """x_obs: normalised f32 [B, C, T_obs, H, W] -> advected [B, C, n_future, H, W] from flow_oracle primitives."""
    b, c, t_obs, h, w = x_obs.shape
    s = np.float32(4.0 * COUNTS_SCALE)
    out = np.empty((b, c, n_future, h, w), np.float32)
    for bi in range(b):
        shared = None
        for ci in range(c):
            if flow_channel is None or shared is None:
                u8 = _u8_reference(x_obs[bi, ci if flow_channel is None else flow_channel], s)
                flow = fo.weighted_average(fo.compute_optical_flow(u8))
                shared = flow
            flow = flow if flow_channel is None else shared
            for k in range(1, n_future + 1):
                out[bi, ci, k - 1] = fo.remap_image(x_obs[bi, ci, -1], flow, float(k), fo.BORDER_REPLICATE, np.nan)
    return out


@pytest.mark.parametrize("flow_channel", [None, 0])
@pytest.mark.parametrize("layout", ["NCTHW", "NTHWC"])
@pytest.mark.parametrize("px", [32, 64])
def test_join_against_the_oracle_chain(device, px, layout, flow_channel):
    """7 observed + 12 future frames of 12 channels, against the chain built from flow_oracle primitives (per (b, c), or
    from channel 0 alone).  Observed slices bit-identical; advected slices in raw counts (|d| * std_c) within the bounds the
    project holds for the config-3 join (tests/test_gpu_headline.py): a flow within 1e-3 px of the oracle's moves a few pixels
    to the next 1/32-px step of cv.remap.

    Measured on MI355X: see DESIGN.md section 3.6b."""
    of = _of()
    b, c, t_obs, n_future = 1, 12, 7, 12
    x, std = _normalised(b, t_obs + n_future, c, px, px, seed=1234 + px)
    ref = _oracle_chain(x[:, :, :t_obs], n_future, flow_channel)
    sat = torch.from_numpy(x).to(device)
    if layout == "NTHWC":
        sat = sat.permute(0, 2, 3, 4, 1).contiguous()
    got = of.replace_future_frames_with_flow(sat, n_future, layout=layout, flow_channel=flow_channel)
    if layout == "NTHWC":
        got = got.permute(0, 4, 1, 2, 3)
    got = got.cpu().numpy()
    assert np.array_equal(got[:, :, :t_obs].view(np.uint32), x[:, :, :t_obs].view(np.uint32))
    assert np.isfinite(got).all()
    d_counts = np.abs(got[:, :, t_obs:] - ref) * std[None, :, None, None, None]
    tag = f"{px}px {layout} flow_channel={flow_channel}"
    _check(f"{tag} advected frames mean |d| [counts]", float(d_counts.mean()), 1e-3)
    _check(f"{tag} advected frames p99.9 |d| [counts]", float(np.quantile(d_counts, 0.999)), 0.05)
    _check(f"{tag} advected frames max |d| [counts]", float(d_counts.max()), 8.0)
    _check(f"{tag} fraction of pixels off by > 0.05 counts", float((d_counts > 0.05).mean()), 1e-3)


# ---- 6. the six models ----------------------------------------------------------------------------------------------------
def _planar_batch(b, c, t5, px, nwp, device, seed=40):
    x, _ = _normalised(b, t5, c, px, px, seed=seed)
    g = torch.Generator().manual_seed(seed)
    t30 = 4
    return {"satellite": {"data": torch.from_numpy(x).to(device)}, "nwp": {"data": nwp(g).to(device)},
            "pv": {"pv_yield": torch.rand(b, t5, 128, generator=g).to(device),
                   "pv_system_row_number": torch.randint(0, 940, (b, 128), generator=g).to(device)},
            "gsp": {"gsp_yield": torch.rand(b, t30, 32, generator=g).to(device),
                    "gsp_id": torch.randint(1, 339, (b, 32), generator=g).to(device)}}


def _dict_batch(b, px, with_coords, device, seed=41):
    from predict_pv_yield_amd.data.seeded import make_fake_sat_batch
    batch = make_fake_sat_batch(b, px, 12, torch.Generator().manual_seed(seed), with_coords, history_len=6, forecast_len=4)
    x, _ = _normalised(b, 11, 12, px, px, seed=seed)
    batch["sat_data"] = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 3, 4, 1)))
    return {k: v.to(device) for k, v in batch.items()}


def _cases():
    from predict_pv_yield_amd.models.conv2d.exp002 import LitModel as Exp002
    from predict_pv_yield_amd.models.conv3d.model_sat_nwp import Model as SatNwp
    from predict_pv_yield_amd.models.perceiver.exp003 import LitModel as Exp003
    from predict_pv_yield_amd.models.perceiver.perceiver import PerceiverModel
    from predict_pv_yield_amd.models.perceiver.perceiver_conv3d_nwp_sat import Model as PerceiverConv3d
    from predict_pv_yield_amd.models.perceiver.perceiver_nwp_sat import Model as PerceiverNwpSat
    pm = dict(history_minutes=30, forecast_minutes=20, batch_size=2, num_latents=16, latent_dim=64)     # 7 observed + 4 future
    return {
        "model_sat_nwp": dict(
            cls=SatNwp, layout="NCTHW", n_future=4, drop=dict(include_future_satellite=False),
            kw=dict(history_minutes=30, forecast_minutes=20, number_of_conv3d_layers=2, image_size_pixels=24,
                    nwp_image_size_pixels=8, number_sat_channels=12, include_pv_yield_history=False, fc1_output_features=16,
                    fc2_output_features=16, fc3_output_features=16),
            batch=lambda dev: _planar_batch(2, 12, 11, 24, lambda g: torch.randn(2, 10, 2, 8, 8, generator=g), dev)),
        "perceiver": dict(
            cls=PerceiverModel, layout="NCTHW", n_future=4, drop=None, kw=pm,
            batch=lambda dev: _planar_batch(2, 11, 11, 24, lambda g: torch.randn(2, 10, 3, 64, 64, generator=g), dev)),
        "perceiver_nwp_sat": dict(
            cls=PerceiverNwpSat, layout="NCTHW", n_future=4, drop=None, kw=pm,
            batch=lambda dev: _planar_batch(2, 11, 11, 24, lambda g: torch.randn(2, 10, 2, 24, 24, generator=g), dev)),
        "perceiver_conv3d_nwp_sat": dict(
            cls=PerceiverConv3d, layout="NCTHW", n_future=4, drop=dict(use_future_satellite_images=False),
            kw=dict(pm, num_latents=12, latent_dim=24, embedding_dem=0, conv3d_channels=8),
            batch=lambda dev: _planar_batch(2, 11, 11, 24, lambda g: torch.randn(2, 10, 11, 24, 24, generator=g), dev)),
        "exp002": dict(cls=Exp002, layout="NTHWC", n_future=4, drop=None, kw=dict(history_len=6, forecast_len=4),
                       batch=lambda dev: _dict_batch(2, 32, True, dev)),
        "exp003": dict(cls=Exp003, layout="NTHWC", n_future=4, drop=None,
                       kw=dict(history_len=6, forecast_len=4, operand_dtype="f32"),
                       batch=lambda dev: _dict_batch(2, 32, False, dev)),
    }


def _sat(batch):
    return batch["sat_data"] if "sat_data" in batch else batch["satellite"]["data"]


def _with_sat(batch, sat):
    if "sat_data" in batch:
        return dict(batch, sat_data=sat)
    return dict(batch, satellite=dict(batch["satellite"], data=sat))


def _twin(case, device, state=None, **knobs):
    torch.manual_seed(19)
    model = case["cls"](**case["kw"], **knobs)
    if state is not None:
        model.load_state_dict(state)
    return model.to(device)


@pytest.mark.parametrize("name", ["model_sat_nwp", "perceiver", "perceiver_nwp_sat", "perceiver_conv3d_nwp_sat", "exp002",
                                  "exp003"])
def test_model_with_the_join(device, name):
    of = _of()
    case = _cases()[name]
    n_future, layout = case["n_future"], case["layout"]
    b_true = _twin(case, device)
    state = {k: v.detach().cpu().clone() for k, v in b_true.state_dict().items()}
    a_flow = _twin(case, device, state, future_frames="optical_flow")
    a_shared = _twin(case, device, state, future_frames="optical_flow", flow_channel=0)
    batch = case["batch"](device)
    sat = _sat(batch)
    t_axis = 2 if layout == "NCTHW" else 1
    with torch.no_grad():
        for model, ch in ((a_flow, None), (a_shared, 0)):
            replaced = of.replace_future_frames_with_flow(sat, n_future, layout=layout, flow_channel=ch)
            y = model(batch)
            assert torch.isfinite(y).all()
            assert torch.equal(y, b_true(_with_sat(batch, replaced))), ch
            # nothing of the true future leaks in
            hidden = sat.clone()
            hidden.narrow(t_axis, sat.shape[t_axis] - n_future, n_future).fill_(float("nan"))
            assert torch.equal(model(_with_sat(batch, hidden)), y), ch
            # a tensor a loader has tagged as advected is taken as it is
            tagged = sat.clone()
            tagged._pv_advected = True
            assert torch.equal(model(_with_sat(batch, tagged)), b_true(batch)), ch
        assert not torch.equal(a_flow(batch), a_shared(batch))
        assert not torch.equal(a_flow(batch), b_true(batch))
        if case["drop"] is not None:
            dropped_flow = _twin(case, device, None, future_frames="optical_flow", **case["drop"])
            dropped_true = _twin(case, device, {k: v.detach().cpu().clone() for k, v in dropped_flow.state_dict().items()},
                                 **case["drop"])
            assert torch.equal(dropped_flow(batch), dropped_true(batch))
    before = sat.clone()
    loss = a_flow.training_step(batch, 0)
    assert torch.isfinite(loss).all()
    loss.backward()
    n_grads = 0
    for k, p in a_flow.named_parameters():
        if p.grad is not None:
            assert torch.isfinite(p.grad).all(), k
            n_grads += 1
    assert n_grads > 0
    assert torch.equal(sat, before)                              # the batch is not modified


# ---- 7. Trainer -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,datamodule,px", [("exp002_cnn_rnn_optical_flow", "exp002_fake", 32),
                                                 ("exp003_perceiver_optical_flow", "exp003_fake", 32)])
def test_trainer_fits_the_optical_flow_configs(device, tmp_path, monkeypatch, model, datamodule, px):
    from predict_pv_yield_amd import hydra_lite as H
    from predict_pv_yield_amd import lightning as pl
    monkeypatch.chdir(tmp_path)
    cfg = H.compose(os.path.join(ROOT, "configs"), "config", [f"model={model}", f"datamodule={datamodule}", "callbacks=none",
                                                              "datamodule.batch_size=2", f"datamodule.image_size_pixels={px}",
                                                              "datamodule.n_train_data=3", "datamodule.n_val_data=1"])
    torch.manual_seed(23)
    lit = H.instantiate(cfg.model)
    assert lit.future_frames == "optical_flow" and lit.flow_channel == 0
    dm = H.instantiate(cfg.datamodule)
    trainer = pl.Trainer(gpus=1, max_epochs=1, limit_train_batches=2, log_every_n_steps=1)
    trainer.fit(lit, datamodule=dm)
    assert trainer.global_step == 2
    metrics = trainer.callback_metrics
    assert np.isfinite(metrics["NMAE/Train_epoch"]) and np.isfinite(metrics["NMAE/Validation_epoch"])
    assert all(torch.isfinite(p).all() for p in lit.parameters())


def test_hip_graph_replay_of_the_join_is_refused_before_capture(device, tmp_path, monkeypatch):
    """HIP-graph replay of a step that computes the flow in forward() is out of scope: Trainer(hip_graph=True) and
    GraphedTrainStep raise one clear error before anything is captured (and before any step has run)."""
    from predict_pv_yield_amd import lightning as pl
    from predict_pv_yield_amd.graphs import GraphedTrainStep
    from predict_pv_yield_amd.models.perceiver.exp003 import FakeExp003Dataset, LitModel
    from predict_pv_yield_amd.optim import HipAdam
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(29)
    model = LitModel(history_len=6, forecast_len=4, operand_dtype="f32", future_frames="optical_flow", flow_channel=0).to(device)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    batch = _dict_batch(2, 32, False, device)
    opt = HipAdam(model.parameters(), lr=5e-4, capturable=True)
    with pytest.raises(RuntimeError, match="HIP-graph replay"):
        GraphedTrainStep(model, opt, batch)
    full = LitModel(operand_dtype="f32", future_frames="optical_flow", flow_channel=0)
    loader = torch.utils.data.DataLoader(FakeExp003Dataset(batch_size=2, image_size_pixels=32, length=2), batch_size=None)
    with pytest.raises(RuntimeError, match="HIP-graph replay"):
        pl.Trainer(gpus=1, max_epochs=1, hip_graph=True).fit(full, loader)
    assert all(torch.equal(v, state[k]) for k, v in model.state_dict().items())      # no step ran
    # the same model trains eagerly
    loss = model.training_step(batch, 0)
    assert torch.isfinite(loss).all()
