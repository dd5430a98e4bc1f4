"""Train-step time of notebooks/05_more_image_inputs.ipynb's LitAutoEncoder (the flow prediction, the t0 image and the flow field
of B x 64 x 64 examples as the four input channels of Conv2d 4 -> 32 -> 32 -> 32; the horizon as the 33rd channel of
ConvTranspose2d 33 -> 32 -> 32 -> 1, all 3x3 at stride 1), eager and replayed as a HIP graph, and the device time of every conv
launch of the step.  The yardstick, in the same process and on the same device, is the general Conv3d f32 route
(pv_conv3d_general_{fwd,bwd_data,bwd_weight}_f32) on the same launch: a Conv2d layer as a (1, 3, 3) Conv3d at depth 1 (the
first layer's four-channel input is materialised outside the timing); a ConvTranspose2d layer as the Conv2d it transposes (its
forward is that conv's data gradient, its data gradient that conv's forward, its weight gradient that conv's with the operands
swapped; the bias gradient is not part of the general route's launch there, and the horizon layer's 33-channel input is
materialised outside the timing).  torch's own kernels are timed alongside for information only: the package never calls them.
Warm-up first, device-side event timing of INNER back-to-back calls per sample, the median of REPS alternating samples (ours,
general, torch, ours, ...), inputs resident before the timed region; the samples' min and max are kept as the spread.  Prints
a table and one JSON line.
   python tools/time_nb05.py [batch=64] [reps=7]"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
import nb_timing as NT
from predict_pv_yield_amd import hip_ops as K
from predict_pv_yield_amd.models.conv2d.nb05_more_inputs import LitAutoEncoder

dev = torch.device("cuda:0")
B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
S = 64
INNER = 2                # back-to-back calls per event pair
STEPS = 100              # train steps per wall-clock window (0.2 s at 2 ms a step)

g = torch.Generator().manual_seed(1)
batch = {"input_images": torch.randn(B, 1, S, S, generator=g).to(dev),
         "T0_IMAGES": torch.randn(B, 1, S, S, generator=g).to(dev),
         "optical_flow": (torch.randn(B, 1, 2, S, S, generator=g) * 3).to(dev),
         "forecast_horizon": ((torch.randint(1, 25, (B,), generator=g).float() * 5 - 62.5) / 34.61).to(dev),
         "target_images": torch.randn(B, 1, S, S, generator=g).to(dev)}

# ---- the train step, eager and replayed (tools/nb_timing.py) ----------------------------------------------------------
model, eager, replay = NT.graph_and_eager(LitAutoEncoder, batch, 0.001, STEPS, warmup=2)
print(NT.step_line("nb05", B, S, eager, replay), flush=True)

# ---- every conv launch of the step -------------------------------------------------------------------------------------
pred, t0 = batch["input_images"].reshape(B, S, S), batch["T0_IMAGES"].reshape(B, S, S)
field, horizon = batch["optical_flow"].reshape(B, 2, S, S), batch["forecast_horizon"]
P = lambda seq, i: (seq[i].weight.detach().contiguous(), seq[i].bias.detach().contiguous())      # noqa: E731
(we0, be0), (we2, be2), (we4, be4) = (P(model.encoder, i) for i in (0, 2, 4))
(wd0, bd0), (wd2, bd2), (wd4, bd4) = (P(model.decoder, i) for i in (0, 2, 4))
x_cat = torch.cat((pred.unsqueeze(1), t0.unsqueeze(1), field), 1).contiguous()
e0 = K.conv2d_ae_inputs_fwd_f32(pred, t0, field, we0, be0)
e2 = K.conv2d_ae_fwd_f32(e0, we2, be2)
e4 = K.conv2d_ae_fwd_f32(e2, we4, be4)
d0 = K.convt2d_ae_horizon_fwd_f32(e4, horizon, wd0, bd0)
d2 = K.convt2d_ae_fwd_f32(d0, wd2, bd2)
d4 = K.convt2d_head_fwd_f32(d2, wd4, bd4)
rnd = lambda t: torch.randn(t.shape, generator=g).to(dev)      # noqa: E731
dy_e0, dy_e2, dy_e4, dy_d0, dy_d2, dy_d4 = (rnd(t) for t in (e0, e2, e4, d0, d2, d4))
e4_33 = torch.cat((e4, horizon.view(-1, 1, 1, 1).expand(B, 1, *e4.shape[2:])), 1).contiguous()
u = lambda t: t.unsqueeze(2)      # noqa: E731  NCHW as NCDHW of depth 1 (a view)


def conv_rows(name, x_full, w, b, dy, ours_fwd, ours_dgrad, ours_wgrad):
    """(name, GFLOP, ours, general, torch) of one Conv2d layer's launches; x_full: the input with every channel materialised."""
    gf = 2 * dy.numel() * w[0].numel() / 1e9
    w5 = w.unsqueeze(2)
    rows = [(f"{name} fwd", gf, ours_fwd, lambda: K.conv3d_general_fwd_f32(u(x_full), w5, b, relu=True),
             lambda: F.conv2d(x_full, w, b))]
    if ours_dgrad is not None:
        rows.append((f"{name} dgrad", gf, ours_dgrad,
                     lambda: K.conv3d_general_bwd_data_f32(u(dy), None, w5, tuple(u(x_full).shape), x_mask=u(x_full)),
                     lambda: torch.nn.grad.conv2d_input(tuple(x_full.shape), w, dy)))
    rows.append((f"{name} wgrad + db", gf, ours_wgrad,
                 lambda: K.conv3d_general_bwd_weight_f32(u(x_full), u(dy), None, tuple(w5.shape)),
                 lambda: torch.nn.grad.conv2d_weight(x_full, tuple(w.shape), dy)))
    return rows


def convt_rows(name, x_full, w, b, dy, ours_fwd, ours_dgrad, ours_wgrad):
    """... of one ConvTranspose2d layer: the general route runs the Conv2d it transposes (w [c_in][c_out][3][3] is that conv's
    [c_out'][c_in'][3][3] as it stands)."""
    gf = 2 * x_full.numel() * w[0].numel() / 1e9
    w5 = w.unsqueeze(2)
    return [(f"{name} fwd", gf, ours_fwd, lambda: K.conv3d_general_bwd_data_f32(u(x_full), None, w5, tuple(u(dy).shape)),
             lambda: F.conv_transpose2d(x_full, w, b)),
            (f"{name} dgrad", gf, ours_dgrad, lambda: K.conv3d_general_fwd_f32(u(dy), w5, None),
             lambda: F.conv2d(dy, w)),
            (f"{name} wgrad + db", gf, ours_wgrad,
             lambda: K.conv3d_general_bwd_weight_f32(u(dy), u(x_full), None, tuple(w5.shape), need_bias=False),
             lambda: torch.nn.grad.conv2d_weight(dy, tuple(w.shape), x_full))]


NEW = ("encoder.0", "decoder.0")      # the layers whose forward and weight gradient run the kernels of conv2d_inputs_f32.hip
cases = []
cases += conv_rows("encoder.0 4->32 (three tensors in place)", x_cat, we0, be0, dy_e0,
                   lambda: K.conv2d_ae_inputs_fwd_f32(pred, t0, field, we0, be0), None,
                   lambda: K.conv2d_ae_inputs_bwd_weight_f32(pred, t0, field, dy_e0, tuple(we0.shape)))
cases += conv_rows("encoder.2 32->32", e0, we2, be2, dy_e2, lambda: K.conv2d_ae_fwd_f32(e0, we2, be2),
                   lambda: K.conv2d_ae_bwd_data_f32(dy_e2, None, we2, e0, tuple(e0.shape)),
                   lambda: K.conv2d_ae_bwd_weight_f32(e0, dy_e2, None, tuple(we2.shape)))
cases += conv_rows("encoder.4 32->32", e2, we4, be4, dy_e4, lambda: K.conv2d_ae_fwd_f32(e2, we4, be4),
                   lambda: K.conv2d_ae_bwd_data_f32(dy_e4, None, we4, e2, tuple(e2.shape)),
                   lambda: K.conv2d_ae_bwd_weight_f32(e2, dy_e4, None, tuple(we4.shape)))
cases += convt_rows("decoder.0 33->32 (horizon synthesised)", e4_33, wd0, bd0, dy_d0,
                    lambda: K.convt2d_ae_horizon_fwd_f32(e4, horizon, wd0, bd0),
                    lambda: K.convt2d_ae_bwd_data_f32(dy_d0, None, wd0[:32], e4, tuple(e4.shape)),
                    lambda: K.convt2d_ae_horizon_bwd_weight_f32(e4, horizon, dy_d0, None, tuple(wd0.shape)))
cases += convt_rows("decoder.2 32->32", d0, wd2, bd2, dy_d2, lambda: K.convt2d_ae_fwd_f32(d0, wd2, bd2),
                    lambda: K.convt2d_ae_bwd_data_f32(dy_d2, None, wd2, d0, tuple(d0.shape)),
                    lambda: K.convt2d_ae_bwd_weight_f32(d0, dy_d2, None, tuple(wd2.shape)))
cases += convt_rows("decoder.4 32->1 (head)", d2, wd4, bd4, dy_d4, lambda: K.convt2d_head_fwd_f32(d2, wd4, bd4),
                    lambda: K.convt2d_head_bwd_data_f32(dy_d4, None, wd4, d2, tuple(d2.shape)),
                    lambda: K.convt2d_head_bwd_weight_f32(d2, dy_d4, None, tuple(wd4.shape)))


rows_out, ratios, tot = [], {}, NT.totals()
print(NT.spread_header(52))
for r in NT.time_cases(cases, REPS, INNER, warmup=2):
    NT.add(tot, r)
    rows_out.append(NT.spread_record(r, new_kernel=r.name.startswith(NEW) and not r.name.endswith("dgrad")))
    if r.general:
        ratios[r.name] = rows_out[-1]["ours_over_general"]
    print(NT.spread_line(r, 52), flush=True)

print(NT.spread_total_line("conv launches of a step (median each, summed)", 52, tot))
print(json.dumps({"tool": "time_nb05", "batch": B, "image": S, "reps": REPS, "calls_per_sample": INNER, "steps_per_window": STEPS,
                  "eager_ms": round(eager * 1e3, 4), "graph_ms": round(replay * 1e3, 4),
                  "samples_per_s_graph": round(B / replay, 2), "step_gflop": round(tot["gflop"], 3),
                  "launches_ours_ms": round(tot["ours"], 4), "launches_general_ms": round(tot["general"], 4),
                  "launches_torch_ms": round(tot["torch"], 4), "time_over_general_route": ratios, "launches": rows_out}))
