"""Train-step time of notebooks/10_just_conv.ipynb's LitAutoEncoder (B x 4 x 128 x 128 normalised frames plus the horizon
stripe, Conv2d 5 -> 64 -> 128 -> 128 (padding 2) -> 1 (stride 2, padding 2)), eager and replayed as a HIP graph, and the device
time of every conv launch of the step with its fraction of the f32 matrix peak.  Alongside, in the same process and on the
same device: the same passes on the general Conv3d f32 route (kernel 1x3x3, padding (0, p, p), stride (1, s, s)) -- the code
path the step would take without csrc/conv2d_wide_f32.hip; the first layer's 5-channel input is materialised outside the
timing -- and torch's own kernels (comparison only: the package never calls them).  Warm-up first, device-side event timing
of INNER back-to-back calls per sample, the median of REPS alternating samples, inputs resident before the timed region.
Passes the general route refuses (128-channel weights beyond its LDS tile) are left out of both sums and named.  Prints a
table and one JSON line; exits non-zero when the compared launches sum to more than the general route's (the
requirement is a ratio <= 1.0).
   python tools/time_nb10.py [batch=64] [reps=10]"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
import nb_timing as NT
from predict_pv_yield_amd import hip_ops as K
from predict_pv_yield_amd.conv2d_functional import STRIPE_WIDTH, stripe_start_from_horizon
from predict_pv_yield_amd.models.conv2d.nb10_just_conv import LitAutoEncoder, output_side

dev = torch.device("cuda:0")
B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
S = 128
T = output_side(S)

g = torch.Generator().manual_seed(1)
batch = {"HISTORICAL_SAT_IMAGES": torch.randn(B, 4, S, S, generator=g).to(dev),
         "FORECAST_HORIZON": torch.randint(1, 24, (B,), generator=g).to(dev),
         "TARGET_SAT_IMAGE": torch.randn(B, T, T, generator=g).to(dev)}

# ---- the train step, eager and replayed (tools/nb_timing.py) ----------------------------------------------------------
model, eager, replay = NT.graph_and_eager(LitAutoEncoder, batch, 0.001, REPS, warmup=3)

# ---- every conv launch of the step -------------------------------------------------------------------------------------
hist = batch["HISTORICAL_SAT_IMAGES"]
start = stripe_start_from_horizon(batch["FORECAST_HORIZON"])
P = lambda i: (model.conv[i].weight.detach().contiguous(), model.conv[i].bias.detach().contiguous())      # noqa: E731
(w1, b1), (w2, b2), (w3, b3), (w4, b4) = (P(i) for i in (0, 2, 4, 6))
y1 = K.conv2d_wide_stripe_fwd_f32(hist, start, w1, b1, STRIPE_WIDTH)
y2 = K.conv2d_wide_fwd_f32(y1, w2, b2, padding=0)
y3 = K.conv2d_wide_fwd_f32(y2, w3, b3, padding=2)
y4 = K.conv2d_head_s2_fwd_f32(y3, w4, b4)
rnd = lambda t: torch.randn(t.shape, generator=g).to(dev)      # noqa: E731
dy4, dy3, dy2, dy1 = (rnd(t) for t in (y4, y3, y2, y1))
cols = torch.arange(S, device=dev).view(1, 1, 1, S)
stripe = ((cols >= start.view(-1, 1, 1, 1)) & (cols < start.view(-1, 1, 1, 1) + STRIPE_WIDTH)).float().expand(B, 1, S, S)
x5 = torch.cat((hist, stripe), 1).contiguous()
v5 = lambda t: t.unsqueeze(2)      # noqa: E731  [N, C, H, W] -> [N, C, 1, H, W] (a view; the kernels take NC(D)HW memory)


def conv_rows(name, x, w, b, dy, pad, stride, relu, ours_fwd, ours_dgrad, ours_wgrad, first=False):
    """(name, GFLOP, ours, general Conv3d route, torch) of one Conv2d layer's launches.  Both routes gate dx by the layer
    input, as the step does."""
    n, ci, h, wd = x.shape
    co = w.shape[0]
    gf = 2 * n * co * ci * 9 * dy.shape[2] * dy.shape[3] / 1e9
    w5, shp5 = v5(w), tuple(v5(x).shape)
    st3, pd3 = (1, stride, stride), (0, pad, pad)
    rows = [(f"{name} fwd", gf, ours_fwd, lambda: K.conv3d_general_fwd_f32(v5(x), w5, b, stride=st3, padding=pd3, relu=relu),
             lambda: F.conv2d(x, w, b, stride=stride, padding=pad))]
    if not first:
        rows.append((f"{name} dgrad", gf, ours_dgrad,
                     lambda: K.conv3d_general_bwd_data_f32(v5(dy), None, w5, shp5, stride=st3, padding=pd3, x_mask=v5(x)),
                     lambda: torch.nn.grad.conv2d_input(tuple(x.shape), w, dy, stride=stride, padding=pad)))
    rows.append((f"{name} wgrad + db", gf, ours_wgrad,
                 lambda: K.conv3d_general_bwd_weight_f32(v5(x), v5(dy), None, tuple(w5.shape), stride=st3, padding=pd3),
                 lambda: torch.nn.grad.conv2d_weight(x, tuple(w.shape), dy, stride=stride, padding=pad)))
    return rows


cases = []
cases += conv_rows("conv.0 5->64 (stripe synthesised while staged)", x5, w1, b1, dy1, 0, 1, True,
                   lambda: K.conv2d_wide_stripe_fwd_f32(hist, start, w1, b1, STRIPE_WIDTH), None,
                   lambda: K.conv2d_wide_stripe_bwd_weight_f32(hist, start, dy1, tuple(w1.shape), STRIPE_WIDTH), first=True)
for nm, x, w, b, dy, pad in (("conv.2 64->128", y1, w2, b2, dy2, 0), ("conv.4 128->128 p2", y2, w3, b3, dy3, 2)):
    cases += conv_rows(nm, x, w, b, dy, pad, 1, True,
                       lambda x=x, w=w, b=b, pad=pad: K.conv2d_wide_fwd_f32(x, w, b, padding=pad),
                       lambda x=x, w=w, dy=dy, pad=pad: K.conv2d_wide_bwd_data_f32(dy, None, w, x, tuple(x.shape), padding=pad),
                       lambda x=x, w=w, dy=dy, pad=pad: K.conv2d_wide_bwd_weight_f32(x, dy, None, tuple(w.shape), padding=pad))
cases += conv_rows("conv.6 128->1 s2 p2 (head)", y3, w4, b4, dy4, 2, 2, False,
                   lambda: K.conv2d_head_s2_fwd_f32(y3, w4, b4),
                   lambda: K.conv2d_head_s2_bwd_data_f32(dy4, None, w4, y3, tuple(y3.shape)),
                   lambda: K.conv2d_head_s2_bwd_weight_f32(y3, dy4, None, tuple(w4.shape)))


INNER = 4      # back-to-back calls per event pair
rows_out, tot = [], NT.totals()
unexpressed, tot_cmp = [], 0.0      # passes the general route refuses: left out of both sums of the ratio, and named
print(NT.step_line("nb10", B, S, eager, replay, digits=0), flush=True)
print(NT.peak_header(50))
for r in NT.time_cases(cases, REPS, INNER, warmup=3, general_name="general Conv3d route"):
    NT.add(tot, r)
    if r.general:
        tot_cmp += r.ours.med
    else:
        unexpressed.append(r.name)
    rows_out.append(NT.peak_record(r))
    print(NT.peak_line(r, 50), flush=True)
ratio = tot_cmp / tot["general"] if tot["general"] > 0 else None
print(f"the step's launches the general Conv3d f32 route can express: {tot_cmp:.3f} ms against its {tot['general']:.3f} ms, "
      f"ratio {ratio} (required <= 1.0); it refuses: {unexpressed}")
print(NT.peak_total_line(50, tot))
print(json.dumps({"tool": "time_nb10", "batch": B, "image": S, "reps": REPS, "eager_ms": round(eager * 1e3, 4),
                  "graph_ms": round(replay * 1e3, 4), "samples_per_s_graph": round(B / replay, 1),
                  "step_gflop": round(tot["gflop"], 2), "step_of_peak_graph": round(tot["gflop"] / replay / 1e3 / NT.PEAK_TFLOPS, 4),
                  "launches_ours_ms": round(tot["ours"], 4), "launches_ours_compared_ms": round(tot_cmp, 4),
                  "general_route_refuses": unexpressed, "launches_general_ms": round(tot["general"], 4),
                  "launches_torch_ms": round(tot["torch"], 4), "ours_over_general": round(ratio, 4) if ratio else None,
                  "calls_per_sample": INNER, "launches": rows_out}))
if ratio is None or ratio > 1.0:
    sys.exit(f"time_nb10: the step's launches take {ratio} x the general Conv3d f32 route's time; the requirement is <= 1.0")
