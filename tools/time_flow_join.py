"""Device time of the optical-flow join of the satellite models (replace_future_frames_with_flow and the models'
future_frames="optical_flow") at the configured sizes of experiment 002, experiment 003 and model_sat_nwp:

  1. the advection alone, per stage (pv_stage_timing), for flow_channel=None (each channel its own flow) and 0 (one flow);
  2. the train step with future_frames "true" and "optical_flow";
  3. the planar prologue of this tree against the chain replace_future_frames_with_flow was before (a contiguous copy, torch
     multiply / add / clamp, u8_from_10bit, a clone of the whole tensor), alternating in one process as tools/ab_models.py does.

   python tools/time_flow_join.py [advect|step|ab|all] [exp003 image size, default 64]

Inputs are data.synthetic.advected_counts normalised with SAT_MEAN / SAT_STD (Farnebäck's iteration count is fixed, its time
does not depend on the texture; the remap's gathers do).  Times are medians over rounds of back-to-back calls between two
HIP events; the spread printed is min..max over the rounds."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from predict_pv_yield_amd import hip_ops as K
from predict_pv_yield_amd import optical_flow as of
from predict_pv_yield_amd.data.synthetic import advected_counts

what = sys.argv[1] if len(sys.argv) > 1 else "all"
px003 = int(sys.argv[2]) if len(sys.argv) > 2 else 64
dev = torch.device("cuda:0")


def normalised(b, t_obs, n_future, c, px, channels_last):
    """[B, C, T, H, W] (or [B, T, H, W, C]) f32: t_obs advected-texture frames; the future slices are noise nobody reads."""
    raw, _ = advected_counts(batch=min(b, 4), t=t_obs, channels=c, h=px, w=px, seed=1234)
    raw = np.concatenate([raw] * ((b + 3) // 4))[:b]
    mean, std = (of.SAT_MEAN[:c], of.SAT_STD[:c]) if c == 12 else (of.SAT_MEAN[1:1 + c], of.SAT_STD[1:1 + c])
    x = (raw.astype(np.float32) - mean[None, None, :, None, None]) / std[None, None, :, None, None]
    x = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1, 3, 4))).to(dev)
    x = torch.cat([x, torch.randn(b, c, n_future, px, px, device=dev)], dim=2)
    return x.permute(0, 2, 3, 4, 1).contiguous() if channels_last else x


def timed(fn, calls=10, rounds=7):
    for _ in range(3):
        fn()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / calls * 1e3)
    return statistics.median(out), min(out), max(out)


def fmt(r):
    return f"{r[0]:9.1f} us  ({r[1]:.1f} .. {r[2]:.1f})"


# (name, batch, observed, future, channels, pixels, layout): configs/datamodule/exp002_fake.yaml, the issue's exp003 size
# (the Perceiver timing tool runs 128 px: second argument) and configs/dataset/conv3d_sat_nwp
SIZES = [("exp002", 32, 7, 12, 12, 32, "NTHWC"), ("exp003", 8, 7, 12, 12, px003, "NTHWC"),
         ("model_sat_nwp", 32, 7, 24, 11, 24, "NCTHW")]


def advection():
    for name, b, t_obs, n_future, c, px, layout in SIZES:
        x = normalised(b, t_obs, n_future, c, px, layout == "NTHWC")
        for ch in (None, 0):
            fn = lambda: of.replace_future_frames_with_flow(x, n_future, layout=layout, flow_channel=ch)
            print(f"{name:14s} B={b} {t_obs}+{n_future} frames {px}x{px}x{c} {layout} flow_channel={ch}: advection {fmt(timed(fn))}")
            iters = 10
            with K.stage_timing() as st:
                for _ in range(iters):
                    fn()
            torch.cuda.synchronize()
            for k, (ms, n) in st.stages.items():
                print(f"      {k:58s} {ms / iters * 1e3:8.1f} us  ({n // iters} launch groups; a HIP event at every boundary)")


def _old_replace(sat_data, n_future, counts_scale=255.0 / 6.0):
    """replace_future_frames_with_flow as it was before the fused prologue (planar input, default arguments)."""
    b, c, t, h, w = sat_data.shape
    t_obs = t - n_future
    obs = sat_data[:, :, :t_obs].contiguous()
    counts = ((obs * (4.0 * counts_scale)) + 512.0).clamp_(0.0, 1020.0)
    u8 = K.u8_from_10bit(counts, 0)
    flows = K.farneback_stack(u8, **of.REFERENCE_FARNEBACK_KWARGS)
    mean_flow = K.flow_weighted_mean(flows.view(b * c, t_obs - 1, h, w, 2))
    out = sat_data.contiguous().clone()
    frame = h * w
    K.remap_bilinear_strided(out.data_ptr() + (t_obs - 1) * frame * 4, t * frame, mean_flow,
                             out.data_ptr() + t_obs * frame * 4, t * frame, frame, b * c, n_future, 1.0, h, w,
                             of.BORDER_REPLICATE, float("nan"))
    return out


def ab():
    for name, b, t_obs, n_future, c, px in (("model_sat_nwp", 32, 7, 24, 11, 24), ("conv3d config 3", 32, 12, 6, 11, 64),
                                            ("exp003 frames, planar", 8, 7, 12, 12, px003)):
        x = normalised(b, t_obs, n_future, c, px, False)
        assert torch.equal(_old_replace(x, n_future), of.replace_future_frames_with_flow(x, n_future))
        arms = {"before": lambda: _old_replace(x, n_future), "now": lambda: of.replace_future_frames_with_flow(x, n_future)}
        res = {k: [] for k in arms}
        for fn in arms.values():
            for _ in range(5):
                fn()
        for _ in range(8):
            for k, fn in arms.items():
                res[k].append(timed(fn, calls=10, rounds=1)[0])
        for k in arms:
            print(f"A/B planar {name:22s} B={b} {t_obs}+{n_future} {px}x{px}x{c} {k:6s}: median {statistics.median(res[k]):9.1f} us   "
                  f"all {[round(v, 1) for v in res[k]]}")


def steps():
    from predict_pv_yield_amd.data.fake import FakeDataConfiguration, make_fake_batch
    from predict_pv_yield_amd.data.seeded import make_fake_sat_batch
    from predict_pv_yield_amd.models.conv2d.exp002 import LitModel as Exp002
    from predict_pv_yield_amd.models.conv3d.model_sat_nwp import Model as SatNwp
    from predict_pv_yield_amd.models.perceiver.exp003 import LitModel as Exp003

    def dict_batch(b, px, with_coords):
        batch = make_fake_sat_batch(b, px, 12, torch.Generator().manual_seed(1), with_coords)
        batch = {k: v.to(dev) for k, v in batch.items()}
        batch["sat_data"] = normalised(b, 7, 12, 12, px, True)
        return batch

    sat_nwp_kw = dict(include_pv_or_gsp_yield_history=True, include_nwp=True, forecast_minutes=120, history_minutes=30,
                      number_of_conv3d_layers=6, image_size_pixels=24, number_sat_channels=11, conv3d_channels=32,
                      output_variable="gsp_yield", include_pv_yield_history=False, include_future_satellite=True)
    fake = make_fake_batch(FakeDataConfiguration(batch_size=32, history_minutes=30, forecast_minutes=120,
                                                 satellite_image_size_pixels=24, nwp_image_size_pixels=64),
                           torch.Generator().manual_seed(1)).to(dev)
    fake.satellite.data = normalised(32, 7, 24, 11, 24, False)
    cases = [("exp002", Exp002, {}, dict_batch(32, 32, True), (None, 0)),
             ("exp003", Exp003, dict(operand_dtype="bf16"), dict_batch(8, px003, False), (None, 0)),
             ("model_sat_nwp", SatNwp, sat_nwp_kw, fake, (None,))]
    for name, cls, kw, batch, channels in cases:
        arms = [("true", None)] + [("optical_flow", ch) for ch in channels]
        for future_frames, ch in arms:
            torch.manual_seed(518)
            model = cls(**kw, future_frames=future_frames, flow_channel=ch).to(dev)
            opt = model.configure_optimizers()

            def step():
                opt.zero_grad(set_to_none=True)
                loss = model.training_step(batch, 0)
                loss.backward()
                opt.step()
            print(f"{name:14s} train step future_frames={future_frames:12s} flow_channel={ch}: {fmt(timed(step, calls=5, rounds=5))}")
            del model, opt


if what in ("advect", "all"):
    advection()
if what in ("ab", "all"):
    ab()
if what in ("step", "all"):
    steps()
