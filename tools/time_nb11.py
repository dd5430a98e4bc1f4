"""Train-step time of notebooks/11_just_conv_and_conv_over_time.ipynb's LitAutoEncoder (each of the four B x 128 x 128 normalised
history frames, with the forecast-horizon stripe as a second channel, through the same Conv2d 2 -> 16 -> 32 -> 32 (padding 2)
-> 1 (stride 2, padding 2), folded into the batch as 4 B images; then three (1, 2) convolutions over the four results per
pixel), eager and replayed as a HIP graph, and the device time of every launch of the step.  The yardstick of the conv
launches, in the same process and on the same device, is the general Conv3d f32 route
(pv_conv3d_general_{fwd,bwd_data,bwd_weight}_f32) on the same launch: a Conv2d layer as a (1, 3, 3) Conv3d at depth 1 with the
layer's stride and padding (the first layer's two-channel input is materialised outside the timing).  A launch the general
route refuses is listed with its message and left out of both sums.  The convolution over time has no counterpart there: its
yardstick is torch's own three (1, 2) Conv2d + ReLU on the same tensors, forward and backward (autograd through a retained
graph).  torch's kernels are timed alongside the conv launches for information only: the package never calls them.
Warm-up first, device-side event timing of INNER back-to-back calls per sample, the median of REPS alternating samples (ours,
general, torch, ours, ...), inputs resident before the timed region; the samples' min and max are kept as the spread.  Prints
a table and one JSON line.
   python tools/time_nb11.py [batch=64] [reps=7]"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
import nb_timing as NT
from predict_pv_yield_amd import hip_ops as K
from predict_pv_yield_amd.conv2d_functional import STRIPE_WIDTH, stripe_start_from_horizon
from predict_pv_yield_amd.models.conv2d.nb11_conv_over_time import LitAutoEncoder, output_side

dev = torch.device("cuda:0")
B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
S = 128
T = output_side(S)
FRAMES = 4
INNER = 2                # back-to-back calls per event pair

g = torch.Generator().manual_seed(1)
batch = {"HISTORICAL_SAT_IMAGES": torch.randn(B, FRAMES, S, S, generator=g).to(dev),
         "FORECAST_HORIZON": torch.randint(1, 24, (B,), generator=g).to(dev),
         "TARGET_SAT_IMAGE": torch.randn(B, T, T, generator=g).to(dev)}

# ---- the train step, eager and replayed (tools/nb_timing.py) ----------------------------------------------------------
model, eager, replay = NT.graph_and_eager(LitAutoEncoder, batch, 0.0001, REPS, warmup=2)
print(NT.step_line("nb11", B, S, eager, replay), flush=True)

# ---- every launch of the step --------------------------------------------------------------------------------------------
hist = batch["HISTORICAL_SAT_IMAGES"]
start = stripe_start_from_horizon(batch["FORECAST_HORIZON"], STRIPE_WIDTH)
P = lambda seq, i: (seq[i].weight.detach().contiguous(), seq[i].bias.detach().contiguous())      # noqa: E731
(w0, b0), (w2, b2), (w4, b4), (w6, b6) = (P(model.conv, i) for i in (0, 2, 4, 6))
tparams = [t for i in (0, 2, 4) for t in P(model.temporal_conv, i)]
a0 = K.conv2d_ae_frame_stripe_fwd_f32(hist, start, w0, b0, STRIPE_WIDTH)
a2 = K.conv2d_ae_fwd_f32(a0, w2, b2)
a4 = K.conv2d_ae_fwd_f32(a2, w4, b4, padding=2)
a6 = K.conv2d_head_s2_fwd_f32(a4, w6, b6, relu=True)
y = K.conv_time_fwd_f32(a6, *tparams)
rnd = lambda t: torch.randn(t.shape, generator=g).to(dev)      # noqa: E731
dy0, dy2, dy4, dy6, dyt = (rnd(t) for t in (a0, a2, a4, a6, y))
# the first layer's input as the general route and torch need it: [4 B, 2, S, S], image 4 b + f
cols = torch.arange(S, device=dev).view(1, 1, 1, 1, S)
plane = ((cols >= start.view(-1, 1, 1, 1, 1)) & (cols < start.view(-1, 1, 1, 1, 1) + STRIPE_WIDTH)).float().expand(B, FRAMES, 1, S, S)
x2 = torch.cat((hist.unsqueeze(2), plane), 2).reshape(B * FRAMES, 2, S, S).contiguous()
u = lambda t: t.unsqueeze(2)      # noqa: E731  NCHW as NCDHW of depth 1 (a view)


def conv_rows(name, x, w, b, dy, stride, pad, ours_fwd, ours_dgrad, ours_wgrad):
    """(name, GFLOP, ours, general, torch) of one Conv2d layer's launches; the general route runs it as a (1, 3, 3) Conv3d at
    depth 1."""
    gf = 2 * dy.numel() * w[0].numel() / 1e9
    w5, st3, pd3 = w.unsqueeze(2), (1, stride, stride), (0, pad, pad)
    rows = [(f"{name} fwd", gf, ours_fwd, lambda: K.conv3d_general_fwd_f32(u(x), w5, b, stride=st3, padding=pd3, relu=True),
             lambda: F.conv2d(x, w, b, stride=stride, padding=pad))]
    if ours_dgrad is not None:
        rows.append((f"{name} dgrad", gf, ours_dgrad,
                     lambda: K.conv3d_general_bwd_data_f32(u(dy), None, w5, tuple(u(x).shape), stride=st3, padding=pd3, x_mask=u(x)),
                     lambda: torch.nn.grad.conv2d_input(tuple(x.shape), w, dy, stride=stride, padding=pad)))
    rows.append((f"{name} wgrad + db", gf, ours_wgrad,
                 lambda: K.conv3d_general_bwd_weight_f32(u(x), u(dy), None, tuple(w5.shape), stride=st3, padding=pd3),
                 lambda: torch.nn.grad.conv2d_weight(x, tuple(w.shape), dy, stride=stride, padding=pad)))
    return rows


cases = []
cases += conv_rows("conv.0 2->16 (4 B images, input synthesised)", x2, w0, b0, dy0, 1, 0,
                   lambda: K.conv2d_ae_frame_stripe_fwd_f32(hist, start, w0, b0, STRIPE_WIDTH), None,
                   lambda: K.conv2d_ae_frame_stripe_bwd_weight_f32(hist, start, dy0, tuple(w0.shape), STRIPE_WIDTH))
N_FIRST = len(cases)
cases += conv_rows("conv.2 16->32 (4 B images)", a0, w2, b2, dy2, 1, 0,
                   lambda: K.conv2d_ae_fwd_f32(a0, w2, b2),
                   lambda: K.conv2d_ae_bwd_data_f32(dy2, None, w2, a0, tuple(a0.shape)),
                   lambda: K.conv2d_ae_bwd_weight_f32(a0, dy2, None, tuple(w2.shape)))
N_PLAIN = len(cases)
cases += conv_rows("conv.4 32->32 padding 2 (4 B images)", a2, w4, b4, dy4, 1, 2,
                   lambda: K.conv2d_ae_fwd_f32(a2, w4, b4, padding=2),
                   lambda: K.conv2d_ae_bwd_data_f32(dy4, None, w4, a2, tuple(a2.shape), padding=2),
                   lambda: K.conv2d_ae_bwd_weight_f32(a2, dy4, None, tuple(w4.shape), padding=2))
N_NEW = len(cases)
NEW = set(range(N_FIRST)) | set(range(N_PLAIN, N_NEW))      # the launches that run the kernels this notebook added
cases += conv_rows("conv.6 32->1 stride 2 padding 2 (head, 4 B images)", a4, w6, b6, dy6, 2, 2,
                   lambda: K.conv2d_head_s2_fwd_f32(a4, w6, b6, relu=True),
                   lambda: K.conv2d_head_s2_bwd_data_f32(dy6, None, w6, a4, tuple(a4.shape)),
                   lambda: K.conv2d_head_s2_bwd_weight_f32(a4, dy6, None, tuple(w6.shape)))

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

# ---- the convolution over time against torch's three (1, 2) Conv2d + ReLU on the same tensors -----------------------------
tw = [t.clone().requires_grad_(True) for t in tparams]
ut = a6.view(B, FRAMES, T * T).permute(0, 2, 1).unsqueeze(1).contiguous().requires_grad_(True)      # the notebook's [B, 1, P, 4]


def torch_head():
    h = F.relu(F.conv2d(ut, tw[0], tw[1]))
    return F.conv2d(F.relu(F.conv2d(h, tw[2], tw[3])), tw[4], tw[5])


yt = torch_head()
dyt_t = dyt.reshape(yt.shape)
pixel_gf = 2 * B * T * T * (16 * 2 * 3 + 16 * 16 * 2 * 2 + 16 * 2) / 1e9
head_cases = [("temporal_conv fwd (3 layers per pixel)", pixel_gf, lambda: K.conv_time_fwd_f32(a6, *tparams), None, torch_head),
              ("temporal_conv bwd (du + 6 parameter gradients)", 2 * pixel_gf,
               lambda: K.conv_time_bwd_f32(a6, dyt, *tparams[:5], True), None,
               lambda: torch.autograd.grad(yt, [ut] + tw, dyt_t, retain_graph=True))]
head_out = []
print(f"{'launch':58s} {'GFLOP':>7s} {'ours ms':>8s} {'spread':>15s} {'torch ms':>9s} {'spread':>15s} {'ours/torch':>10s}")
for r in NT.time_cases(head_cases, REPS, INNER, warmup=2):
    ours_all += r.ours.med
    head_out.append({"launch": r.name, "new_kernel": True, "gflop": round(r.gflop, 4), "ours_ms": NT.r4(r.ours.med),
                     "ours_ms_min": NT.r4(r.ours.lo), "ours_ms_max": NT.r4(r.ours.hi), "torch_ms": NT.r4(r.torch.med),
                     "torch_ms_min": NT.r4(r.torch.lo), "torch_ms_max": NT.r4(r.torch.hi),
                     "ours_over_torch": round(r.ours.med / r.torch.med, 4)})
    print(f"{r.name:58s} {r.gflop:7.3f} {r.ours.med:8.3f} {NT.spread(r.ours)} {r.torch.med:9.3f} {NT.spread(r.torch)} "
          f"{r.ours.med / r.torch.med:10.3f}", flush=True)

print(json.dumps({"tool": "time_nb11", "batch": B, "image": S, "reps": REPS, "calls_per_sample": INNER,
                  "eager_ms": round(eager * 1e3, 4), "graph_ms": round(replay * 1e3, 4),
                  "samples_per_s_graph": round(B / replay, 2), "compared_gflop": round(tot["gflop"], 3),
                  "launches_ours_ms": round(tot["ours"], 4), "launches_general_ms": round(tot["general"], 4),
                  "launches_torch_ms": round(tot["torch"], 4), "all_launches_ours_ms": round(ours_all, 4),
                  "refused_by_general_route": refused, "time_over_general_route": ratios, "launches": rows_out,
                  "conv_over_time": head_out}))
