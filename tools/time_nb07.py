"""Train-step time of notebooks/07_multiple_historical_images.ipynb's LitAutoEncoder (each of the four B x 128 x 128 normalised
history frames, with the horizon as a second channel, through the same Conv2d 2 -> 32 -> 32 -> 32 stride-2 encoder, folded
into the batch as 4 B images; ConvTranspose2d 128 -> 32 -> 32 -> 1), eager and replayed as a HIP graph, and the device time of
every conv launch of the step.  The yardstick, in the same process and on the same device, is the general Conv3d f32 route
(pv_conv3d_general_{fwd,bwd_data,bwd_weight}_f32) on the same launch: a Conv2d layer as a (1, 3, 3) Conv3d at depth 1 (the
first layer's two-channel input is materialised outside the timing); a ConvTranspose2d layer as the Conv2d it transposes
(its forward is that conv's data gradient, its data gradient that conv's forward, its weight gradient that conv's with the
operands swapped; the bias gradient is not part of the general route's launch there).  A launch the general route refuses
is listed with its message and left out of both sums.  torch's own kernels are timed alongside for information only: the
package never calls them.
Warm-up first, device-side event timing of INNER back-to-back calls per sample, the median of REPS alternating samples (ours,
general, torch, ours, ...), inputs resident before the timed region; the samples' min and max are kept as the spread.  Prints
a table and one JSON line.
   python tools/time_nb07.py [batch=64] [reps=7]"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
import nb_timing as NT
from predict_pv_yield_amd import hip_ops as K
from predict_pv_yield_amd.models.conv2d.nb07_multi_hist import LitAutoEncoder, target_side

dev = torch.device("cuda:0")
B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
S = 128
T = target_side(S)
FRAMES = 4
INNER = 2                # back-to-back calls per event pair

g = torch.Generator().manual_seed(1)
batch = {"HISTORICAL_SAT_IMAGES": torch.randn(B, FRAMES, S, S, generator=g).to(dev),
         "FORECAST_HORIZON": ((torch.randint(1, 25, (B,), generator=g).float() - 12.5) / 6.9222).to(dev),
         "TARGET_SAT_IMAGE": torch.randn(B, T, T, generator=g).to(dev)}

# ---- the train step, eager and replayed (tools/nb_timing.py) ----------------------------------------------------------
model, eager, replay = NT.graph_and_eager(LitAutoEncoder, batch, 0.001, REPS, warmup=2)
print(NT.step_line("nb07", B, S, eager, replay), flush=True)

# ---- every conv launch of the step -------------------------------------------------------------------------------------
hist, horizon = batch["HISTORICAL_SAT_IMAGES"], batch["FORECAST_HORIZON"]
P = lambda seq, i: (seq[i].weight.detach().contiguous(), seq[i].bias.detach().contiguous())      # noqa: E731
(we0, be0), (we2, be2), (we4, be4) = (P(model.encoder_conv, i) for i in (0, 2, 4))
(wd0, bd0), (wd2, bd2), (wd4, bd4) = (P(model.decoder_conv, i) for i in (0, 2, 4))
e0 = K.conv2d_s2_frame_horizon_fwd_f32(hist, horizon, we0, be0)
e2 = K.conv2d_s2_fwd_f32(e0, we2, be2)
e4 = K.conv2d_s2_fwd_f32(e2, we4, be4)
enc = e4.view(B, FRAMES * e4.shape[1], *e4.shape[2:])
d0 = K.convt2d_s2_frames_fwd_f32(enc, wd0, bd0)
d2 = K.convt2d_s2_fwd_f32(d0, wd2, bd2)
d4 = K.convt2d_head_fwd_f32(d2, wd4, bd4)
rnd = lambda t: torch.randn(t.shape, generator=g).to(dev)      # noqa: E731
dy_e0, dy_e2, dy_e4, dy_d0, dy_d2, dy_d4 = (rnd(t) for t in (e0, e2, e4, d0, d2, d4))
# the first layer's input as the general route and torch need it: [4 B, 2, S, S], image 4 b + f
x2 = torch.cat((hist.unsqueeze(2), horizon.view(-1, 1, 1, 1, 1).expand(B, FRAMES, 1, S, S)), 2).reshape(B * FRAMES, 2, S, S).contiguous()
u = lambda t: t.unsqueeze(2)      # noqa: E731  NCHW as NCDHW of depth 1 (a view)
ST = (1, 2, 2)


def conv_rows(name, x, w, b, dy, ours_fwd, ours_dgrad, ours_wgrad):
    """(name, GFLOP, ours, general, torch) of one stride-2 Conv2d layer's launches; the general route runs it as a (1, 3, 3)
    Conv3d at depth 1."""
    gf = 2 * dy.numel() * w[0].numel() / 1e9
    w5 = w.unsqueeze(2)
    rows = [(f"{name} fwd", gf, ours_fwd, lambda: K.conv3d_general_fwd_f32(u(x), w5, b, stride=ST, relu=True),
             lambda: F.conv2d(x, w, b, stride=2))]
    if ours_dgrad is not None:
        rows.append((f"{name} dgrad", gf, ours_dgrad,
                     lambda: K.conv3d_general_bwd_data_f32(u(dy), None, w5, tuple(u(x).shape), stride=ST, x_mask=u(x)),
                     lambda: torch.nn.grad.conv2d_input(tuple(x.shape), w, dy, stride=2)))
    rows.append((f"{name} wgrad + db", gf, ours_wgrad,
                 lambda: K.conv3d_general_bwd_weight_f32(u(x), u(dy), None, tuple(w5.shape), stride=ST),
                 lambda: torch.nn.grad.conv2d_weight(x, tuple(w.shape), dy, stride=2)))
    return rows


def convt_rows(name, x, w, b, dy, stride, ours_fwd, ours_dgrad, ours_wgrad):
    """... of one ConvTranspose2d layer: the general route runs the Conv2d it transposes (w [c_in][c_out][3][3] is that conv's
    [c_out'][c_in'][3][3] as it stands)."""
    gf = 2 * x.numel() * w[0].numel() / 1e9
    w5, st3 = w.unsqueeze(2), (1, stride, stride)
    return [(f"{name} fwd", gf, ours_fwd,
             lambda: K.conv3d_general_bwd_data_f32(u(x), None, w5, tuple(u(dy).shape), stride=st3),
             lambda: F.conv_transpose2d(x, w, b, stride=stride)),
            (f"{name} dgrad", gf, ours_dgrad, lambda: K.conv3d_general_fwd_f32(u(dy), w5, None, stride=st3),
             lambda: F.conv2d(dy, w, stride=stride)),
            (f"{name} wgrad + db", gf, ours_wgrad,
             lambda: K.conv3d_general_bwd_weight_f32(u(dy), u(x), None, tuple(w5.shape), stride=st3, need_bias=False),
             lambda: torch.nn.grad.conv2d_weight(dy, tuple(w.shape), x, stride=stride))]


cases = []
cases += conv_rows("encoder_conv.0 2->32 s2 (4 B images, input synthesised)", x2, we0, be0, dy_e0,
                   lambda: K.conv2d_s2_frame_horizon_fwd_f32(hist, horizon, we0, be0), None,
                   lambda: K.conv2d_s2_frame_horizon_bwd_weight_f32(hist, horizon, dy_e0, tuple(we0.shape)))
N_FIRST = len(cases)
cases += conv_rows("encoder_conv.2 32->32 s2 (4 B images)", e0, we2, be2, dy_e2,
                   lambda: K.conv2d_s2_fwd_f32(e0, we2, be2),
                   lambda: K.conv2d_s2_bwd_data_f32(dy_e2, None, we2, e0, tuple(e0.shape)),
                   lambda: K.conv2d_s2_bwd_weight_f32(e0, dy_e2, None, tuple(we2.shape)))
cases += conv_rows("encoder_conv.4 32->32 s2 (4 B images)", e2, we4, be4, dy_e4,
                   lambda: K.conv2d_s2_fwd_f32(e2, we4, be4),
                   lambda: K.conv2d_s2_bwd_data_f32(dy_e4, None, we4, e2, tuple(e2.shape)),
                   lambda: K.conv2d_s2_bwd_weight_f32(e2, dy_e4, None, tuple(we4.shape)))
N_ENC = len(cases)
cases += convt_rows("decoder_conv.0 128->32 s2 (frame seam)", enc, wd0, bd0, dy_d0, 2,
                    lambda: K.convt2d_s2_frames_fwd_f32(enc, wd0, bd0),
                    lambda: K.convt2d_s2_frames_bwd_data_f32(dy_d0, None, wd0, enc, tuple(enc.shape)),
                    lambda: K.convt2d_s2_frames_bwd_weight_f32(enc, dy_d0, None, tuple(wd0.shape)))
N_NEW = len(cases)
NEW = set(range(N_FIRST)) | set(range(N_ENC, N_NEW))      # the launches that run the kernels of csrc/conv2d_frames_f32.hip
cases += convt_rows("decoder_conv.2 32->32 s2", d0, wd2, bd2, dy_d2, 2,
                    lambda: K.convt2d_s2_fwd_f32(d0, wd2, bd2),
                    lambda: K.convt2d_s2_bwd_data_f32(dy_d2, None, wd2, d0, tuple(d0.shape)),
                    lambda: K.convt2d_s2_bwd_weight_f32(d0, dy_d2, None, tuple(wd2.shape)))
cases += convt_rows("decoder_conv.4 32->1 s1 (head)", d2, wd4, bd4, dy_d4, 1,
                    lambda: K.convt2d_head_fwd_f32(d2, wd4, bd4),
                    lambda: K.convt2d_head_bwd_data_f32(dy_d4, None, wd4, d2, tuple(d2.shape)),
                    lambda: K.convt2d_head_bwd_weight_f32(d2, dy_d4, None, tuple(wd4.shape)))


rows_out, ratios, refused, tot, ours_all = [], {}, {}, NT.totals(), 0.0
print(NT.spread_header(58))
for i, r in enumerate(NT.time_cases(cases, REPS, INNER, warmup=2)):
    ours_all += r.ours.med
    rows_out.append(NT.spread_record(r, new_kernel=i in NEW))
    if r.general:                  # a refused launch is left out of both sums
        NT.add(tot, r)
        ratios[r.name] = rows_out[-1]["ours_over_general"]
    else:
        refused[r.name] = r.why_general
    print(NT.spread_line(r, 58), flush=True)

print(NT.spread_total_line("conv launches the general route takes (median each, summed)", 58, tot))
print(json.dumps({"tool": "time_nb07", "batch": B, "image": S, "reps": REPS, "calls_per_sample": INNER,
                  "eager_ms": round(eager * 1e3, 4), "graph_ms": round(replay * 1e3, 4),
                  "samples_per_s_graph": round(B / replay, 2), "compared_gflop": round(tot["gflop"], 3),
                  "launches_ours_ms": round(tot["ours"], 4), "launches_general_ms": round(tot["general"], 4),
                  "launches_torch_ms": round(tot["torch"], 4), "all_launches_ours_ms": round(ours_all, 4),
                  "refused_by_general_route": refused, "time_over_general_route": ratios, "launches": rows_out}))
