"""Train-step time of notebooks/15_int16.ipynb's LitAutoEncoder (B x (4 + 1) x 128 x 128 raw counts, stride-2 Conv2d 6 -> 16 ->
32 -> 32 -> 32, stride-2 ConvTranspose2d 32 -> 32 -> 16 -> 1), eager and replayed as a HIP graph, and the device time of every
conv launch of the step with its fraction of the f32 matrix peak.  Alongside, in the same process and on the same device: the
same passes on the general Conv3d f32 route (kernel 1x3x3, stride 1x2x2) wherever it can express them -- a Conv2d's three
passes as they stand (the 6-channel input materialised outside the timing); a ConvTranspose2d's forward as the data
gradient of the convolution with the same weight tensor (no bias, no ReLU: the route has no epilogue there), its data
gradient as that convolution's forward (no dy gate) and its weight gradient as that convolution's with x and dy swapped (no
bias gradient) -- and torch's own kernels (comparison only: the package never calls them).  Warm-up first, device-side
event timing of INNER back-to-back calls per sample, the median of REPS alternating samples, inputs resident before the
timed region.  Prints a table and one JSON line; exits non-zero when the step's launches sum to more than the general
route's (the requirement is a ratio <= 1.0).
   python tools/time_nb15.py [batch=64] [reps=20]"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
import nb_timing as NT
from predict_pv_yield_amd import hip_ops as K
from predict_pv_yield_amd.models.conv2d.nb15_strided_ae import LitAutoEncoder, target_side

dev = torch.device("cuda:0")
B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
S = 128
T = target_side(S)
S2 = (1, 2, 2)

g = torch.Generator().manual_seed(1)
batch = {"HISTORICAL_SAT_IMAGES": torch.randint(0, 1024, (B, 4, S, S), generator=g).to(torch.int16).to(dev),
         "OPTICAL_FLOW_PREDICTIONS": (torch.randint(0, 1024, (B, S, S), generator=g).float()
                                      + torch.rand(B, S, S, generator=g)).to(dev),
         "FORECAST_HORIZON": torch.randn(B, generator=g).to(dev),
         "TARGET_SAT_IMAGE": torch.randint(0, 1024, (B, T, T), generator=g).to(torch.int16).to(dev)}

# ---- the train step, eager and replayed (tools/nb_timing.py) ----------------------------------------------------------
model, eager, replay = NT.graph_and_eager(LitAutoEncoder, batch, 0.001, REPS, warmup=3)

# ---- every conv launch of the step -------------------------------------------------------------------------------------
hist, flow, hor = batch["HISTORICAL_SAT_IMAGES"], batch["OPTICAL_FLOW_PREDICTIONS"], batch["FORECAST_HORIZON"]
P = lambda i: (model.conv[i].weight.detach().contiguous(), model.conv[i].bias.detach().contiguous())      # noqa: E731
(w1, b1), (w2, b2), (w3, b3), (w4, b4) = (P(i) for i in (0, 2, 4, 6))
(u1, c1), (u2, c2), (u3, c3) = (P(i) for i in (8, 10, 12))
y1 = K.conv2d_s2_counts_fwd_f32(hist, flow, hor, w1, b1)
y2 = K.conv2d_s2_fwd_f32(y1, w2, b2)
y3 = K.conv2d_s2_fwd_f32(y2, w3, b3)
y4 = K.conv2d_s2_fwd_f32(y3, w4, b4)
z1 = K.convt2d_s2_fwd_f32(y4, u1, c1)
z2 = K.convt2d_s2_fwd_f32(z1, u2, c2)
z3 = K.convt2d_s2_fwd_f32(z2, u3, c3, relu=False)
rnd = lambda t: torch.randn(t.shape, generator=g).to(dev)      # noqa: E731
dz3, dz2, dz1, dy4, dy3, dy2, dy1 = (rnd(t) for t in (z3, z2, z1, y4, y3, y2, y1))
x6 = torch.cat(((torch.cat((hist.float(), flow[:, None]), 1) - 93.23458) / 115.34247,
                hor.view(-1, 1, 1, 1).expand(B, 1, S, S)), 1).contiguous()
v5 = lambda t: t.unsqueeze(2)      # noqa: E731  [N, C, H, W] -> [N, C, 1, H, W] (a view; the kernels take NC(D)HW memory)


def conv_rows(name, x, w, b, dy, ours_fwd, ours_dgrad, ours_wgrad, first=False):
    """(name, GFLOP, ours, general Conv3d route, torch) of one Conv2d layer's launches.  Both routes gate dx by the layer
    input, as the step does."""
    n, ci, h, wd = x.shape
    co = w.shape[0]
    gf = 2 * n * co * ci * 9 * dy.shape[2] * dy.shape[3] / 1e9
    w5, shp5 = v5(w), tuple(v5(x).shape)
    rows = [(f"{name} fwd", gf, ours_fwd, lambda: K.conv3d_general_fwd_f32(v5(x), w5, b, stride=S2, relu=True),
             lambda: F.conv2d(x, w, b, stride=2))]
    if not first:
        rows.append((f"{name} dgrad", gf, ours_dgrad,
                     lambda: K.conv3d_general_bwd_data_f32(v5(dy), None, w5, shp5, stride=S2, x_mask=v5(x)),
                     lambda: torch.nn.grad.conv2d_input(tuple(x.shape), w, dy, stride=2)))
    rows.append((f"{name} wgrad + db", gf, ours_wgrad,
                 lambda: K.conv3d_general_bwd_weight_f32(v5(x), v5(dy), None, tuple(w5.shape), stride=S2),
                 lambda: torch.nn.grad.conv2d_weight(x, tuple(w.shape), dy, stride=2)))
    return rows


def convt_rows(name, x, u, b, dy, relu):
    n, ci, h, wd = x.shape
    co = u.shape[1]
    gf = 2 * n * co * ci * 9 * h * wd / 1e9
    u5, yshp5 = v5(u), tuple(v5(dy).shape)
    return [
        (f"{name} fwd", gf, lambda: K.convt2d_s2_fwd_f32(x, u, b, relu=relu),
         lambda: K.conv3d_general_bwd_data_f32(v5(x), None, u5, yshp5, stride=S2), lambda: F.conv_transpose2d(x, u, b, stride=2)),
        (f"{name} dgrad", gf, lambda: K.convt2d_s2_bwd_data_f32(dy, None, u, x, tuple(x.shape)),
         lambda: K.conv3d_general_fwd_f32(v5(dy), u5, None, stride=S2), lambda: F.conv2d(dy, u, stride=2)),
        (f"{name} wgrad + db", gf, lambda: K.convt2d_s2_bwd_weight_f32(x, dy, None, tuple(u.shape)),
         lambda: K.conv3d_general_bwd_weight_f32(v5(dy), v5(x), None, tuple(u5.shape), stride=S2, need_bias=False),
         lambda: torch.nn.grad.conv2d_weight(dy, tuple(u.shape), x, stride=2)),
    ]


cases = []
cases += conv_rows("conv.0 6->16 (counts normalised while staged)", x6, w1, b1, dy1,
                   lambda: K.conv2d_s2_counts_fwd_f32(hist, flow, hor, w1, b1), None,
                   lambda: K.conv2d_s2_counts_bwd_weight_f32(hist, flow, hor, dy1, tuple(w1.shape)), first=True)
for nm, x, w, b, dy in (("conv.2 16->32", y1, w2, b2, dy2), ("conv.4 32->32", y2, w3, b3, dy3), ("conv.6 32->32", y3, w4, b4, dy4)):
    cases += conv_rows(nm, x, w, b, dy, lambda x=x, w=w, b=b: K.conv2d_s2_fwd_f32(x, w, b),
                       lambda x=x, w=w, dy=dy: K.conv2d_s2_bwd_data_f32(dy, None, w, x, tuple(x.shape)),
                       lambda x=x, w=w, dy=dy: K.conv2d_s2_bwd_weight_f32(x, dy, None, tuple(w.shape)))
cases += convt_rows("conv.8 T 32->32", y4, u1, c1, dz1, True)
cases += convt_rows("conv.10 T 32->16", z1, u2, c2, dz2, True)
cases += convt_rows("conv.12 T 16->1", z2, u3, c3, dz3, False)


INNER = 8      # back-to-back calls per event pair: the small launches are microseconds each
rows_out, tot = [], NT.totals()
print(NT.step_line("nb15", B, S, eager, replay, digits=0), flush=True)
print(NT.peak_header(50))
for r in NT.time_cases(cases, REPS, INNER, warmup=3, general_name="general Conv3d route"):
    NT.add(tot, r)
    rows_out.append(NT.peak_record(r))
    print(NT.peak_line(r, 50), flush=True)
ratio = tot["ours"] / tot["general"] if all(row["general_ms"] is not None for row in rows_out) and tot["general"] > 0 else None
print(f"sum of the step's launches / the same passes on the general Conv3d f32 route: {ratio} (required <= 1.0)")
print(NT.peak_total_line(50, tot))
print(json.dumps({"tool": "time_nb15", "batch": B, "image": S, "reps": REPS, "eager_ms": round(eager * 1e3, 4),
                  "graph_ms": round(replay * 1e3, 4), "samples_per_s_graph": round(B / replay, 1),
                  "step_gflop": round(tot["gflop"], 2), "step_of_peak_graph": round(tot["gflop"] / replay / 1e3 / NT.PEAK_TFLOPS, 4),
                  "launches_ours_ms": round(tot["ours"], 4), "launches_general_ms": round(tot["general"], 4),
                  "launches_torch_ms": round(tot["torch"], 4), "ours_over_general": round(ratio, 4) if ratio else None,
                  "calls_per_sample": INNER, "launches": rows_out}))
if ratio is None or ratio > 1.0:
    sys.exit(f"time_nb15: the step's launches take {ratio} x the general Conv3d f32 route's time; the requirement is <= 1.0")
