"""Train-step time of notebooks/16_maxpool.ipynb's LitAutoEncoder (B x (4 + 1) x 128 x 128 raw counts, Conv2d 6 -> 16 -> 32 ->
32 -> 32, MaxPool2d(3), ConvTranspose2d 32 -> 32 -> 16 -> 16 -> 1), eager and replayed as a HIP graph, and the device time of
every conv launch of the step with its fraction of the f32 matrix peak.  Alongside, in the same process and on the same
device: the same layers on the general Conv3d f32 route (kernel 1x3x3; the decoder layers as their equivalent convolutions
over the input padded by 2 with mirrored, channel-swapped weights; the 6-channel input and the pre-pool gradient
materialised outside the timing) -- what the library could do for these layers before csrc/conv2d_ae_f32.hip -- and torch's
own F.conv2d / F.conv_transpose2d (comparison only: the package never calls them).  Warm-up first, device-side event
timing of INNER back-to-back calls per sample, the median of REPS alternating samples, inputs resident before the timed region.  Prints a table and one JSON
line; exits non-zero when the step's launches sum to more than the general route's (the requirement is a ratio <= 1.0).
   python tools/time_nb16.py [batch=64] [reps=20]"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
import nb_timing as NT
from predict_pv_yield_amd import hip_ops as K
from predict_pv_yield_amd.models.conv2d.nb16_maxpool import LitAutoEncoder

dev = torch.device("cuda:0")
B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
S, T = 128, 64

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
P = lambda m: (m.weight.detach().contiguous(), m.bias.detach().contiguous())      # noqa: E731
(w1, b1), (w2, b2), (w3, b3), (w4, b4) = (P(m) for m in (model.encoder_conv1, model.encoder_conv2, model.encoder_conv3,
                                                        model.encoder_conv4))
(u1, c1), (u2, c2), (u3, c3), (u4, c4) = (P(m) for m in (model.decoder_conv1, model.decoder_conv2, model.decoder_conv3,
                                                        model.decoder_conv4))
y1 = K.conv2d_ae_counts_fwd_f32(hist, flow, hor, w1, b1)
y2 = K.conv2d_ae_fwd_f32(y1, w2, b2)
y3 = K.conv2d_ae_fwd_f32(y2, w3, b3)
yp, codes = K.conv2d_ae_pool_fwd_f32(y3, w4, b4)
z1 = K.convt2d_ae_fwd_f32(yp, u1, c1)
z2 = K.convt2d_ae_fwd_f32(z1, u2, c2)
z3 = K.convt2d_ae_fwd_f32(z2, u3, c3)
z4 = K.convt2d_ae_fwd_f32(z3, u4, c4, relu=False)
rnd = lambda t: torch.randn(t.shape, generator=g).to(dev)      # noqa: E731
dz4, dz3, dz2, dz1, dyp, dy3, dy2, dy1 = (rnd(t) for t in (z4, z3, z2, z1, yp, y3, y2, y1))
# operands of the comparison routes, materialised once: the 6-channel input, the pre-pool gradient, 5-d views, the
# decoder weights as the weights of their equivalent convolutions
x6 = torch.cat(((torch.cat((hist.float(), flow[:, None]), 1) - 93.23458) / 115.34247,
                hor.view(-1, 1, 1, 1).expand(B, 1, S, S)), 1).contiguous()
dpre4 = torch.randn(B, 32, S - 8, S - 8, generator=g).to(dev)
v5 = lambda t: t.unsqueeze(2)      # noqa: E731  [N, C, H, W] -> [N, C, 1, H, W] (a view; the kernels take NC(D)HW memory)
eq = lambda u: u.flip(2, 3).transpose(0, 1).contiguous()      # noqa: E731  ConvTranspose2d weight -> equivalent Conv2d weight
e1, e2, e3, e4 = eq(u1), eq(u2), eq(u3), eq(u4)
PADT = (0, 2, 2)


R = " [general route]"


def conv_rows(name, x, w, b, y, dy, ours_fwd, ours_dgrad, ours_wgrad, relu=True, first=False, routed=("", "", "")):
    """(name, GFLOP, ours, general Conv3d route, torch) of one Conv2d layer's launches; routed: per pass (fwd, dgrad, wgrad),
    R where the entry point itself runs the general kernel at this size (>= 32768 output positions; the pooled layer's
    'ours' then includes its pool / expansion kernel).  Both routes gate dx by the layer input, as the step does."""
    n, ci, h, wd = x.shape
    co = w.shape[0]
    gf = 2 * n * co * ci * 9 * (h - 2) * (wd - 2) / 1e9
    w5, shp5 = v5(w), tuple(v5(x).shape)
    rows = [(f"{name} fwd{routed[0]}", gf, ours_fwd, lambda: K.conv3d_general_fwd_f32(v5(x), w5, b, relu=relu),
             lambda: F.conv2d(x, w, b))]
    if not first:
        rows.append((f"{name} dgrad{routed[1]}", gf, ours_dgrad,
                     lambda: K.conv3d_general_bwd_data_f32(v5(dy), None, w5, shp5, x_mask=v5(x)),
                     lambda: torch.nn.grad.conv2d_input(tuple(x.shape), w, dy)))
    rows.append((f"{name} wgrad + db{routed[2]}", gf, ours_wgrad,
                 lambda: K.conv3d_general_bwd_weight_f32(v5(x), v5(dy), None, tuple(w5.shape)),
                 lambda: torch.nn.grad.conv2d_weight(x, tuple(w.shape), dy)))
    return rows


def convt_rows(name, x, u, e, b, dy, relu):
    n, ci, h, wd = x.shape
    co = u.shape[1]
    gf = 2 * n * co * ci * 9 * h * wd / 1e9
    e5, shp5 = v5(e), tuple(v5(x).shape)
    return [
        (f"{name} fwd", gf, lambda: K.convt2d_ae_fwd_f32(x, u, b, relu=relu),
         lambda: K.conv3d_general_fwd_f32(v5(x), e5, b, padding=PADT, relu=relu), lambda: F.conv_transpose2d(x, u, b)),
        (f"{name} dgrad", gf, lambda: K.convt2d_ae_bwd_data_f32(dy, None, u, x, tuple(x.shape)),
         lambda: K.conv3d_general_bwd_data_f32(v5(dy), None, e5, shp5, padding=PADT, x_mask=v5(x)), lambda: F.conv2d(dy, u)),
        (f"{name} wgrad + db", gf, lambda: K.convt2d_ae_bwd_weight_f32(x, dy, None, tuple(u.shape)),
         lambda: K.conv3d_general_bwd_weight_f32(v5(x), v5(dy), None, tuple(e5.shape), padding=PADT),
         lambda: torch.nn.grad.conv2d_weight(dy, tuple(u.shape), x)),
    ]


cases = []
cases += conv_rows("encoder_conv1 6->16 (counts normalised while staged)", x6, w1, b1, y1, dy1,
                   lambda: K.conv2d_ae_counts_fwd_f32(hist, flow, hor, w1, b1), None,
                   lambda: K.conv2d_ae_counts_bwd_weight_f32(hist, flow, hor, dy1, tuple(w1.shape)), first=True)
cases += conv_rows("encoder_conv2 16->32", y1, w2, b2, y2, dy2, lambda: K.conv2d_ae_fwd_f32(y1, w2, b2),
                   lambda: K.conv2d_ae_bwd_data_f32(dy2, None, w2, y1, tuple(y1.shape)),
                   lambda: K.conv2d_ae_bwd_weight_f32(y1, dy2, None, tuple(w2.shape)), routed=("", R, R))
cases += conv_rows("encoder_conv3 32->32", y2, w3, b3, y3, dy3, lambda: K.conv2d_ae_fwd_f32(y2, w3, b3),
                   lambda: K.conv2d_ae_bwd_data_f32(dy3, None, w3, y2, tuple(y2.shape)),
                   lambda: K.conv2d_ae_bwd_weight_f32(y2, dy3, None, tuple(w3.shape)), routed=(R, R, R))
cases += conv_rows("encoder_conv4 32->32 + pool (pooled dy expanded by codes)", y3, w4, b4, None, dpre4,
                   lambda: K.conv2d_ae_pool_fwd_f32(y3, w4, b4),
                   lambda: K.conv2d_ae_pool_bwd_data_f32(dyp, codes, w4, y3, tuple(y3.shape)),
                   lambda: K.conv2d_ae_pool_bwd_weight_f32(y3, dyp, codes, tuple(w4.shape)), routed=(R, "", R))
cases += convt_rows("decoder_conv1 T 32->32", yp, u1, e1, c1, dz1, True)
cases += convt_rows("decoder_conv2 T 32->16", z1, u2, e2, c2, dz2, True)
cases += convt_rows("decoder_conv3 T 16->16", z2, u3, e3, c3, dz3, True)
cases += convt_rows("decoder_conv4 T 16->1", z3, u4, e4, c4, dz4, False)


INNER = 8      # back-to-back calls per event pair: the small decoder launches are microseconds each
rows_out, tot, new = [], NT.totals(), NT.totals()      # new: the launches that run csrc/conv2d_ae_f32.hip's own kernels
print(NT.step_line("nb16", B, S, eager, replay, digits=0), flush=True)
print(NT.peak_header(62))
for r in NT.time_cases(cases, REPS, INNER, warmup=3, general_name="general Conv3d route"):
    routed = r.name.endswith(R)      # the entry point itself runs the general kernel at this size
    NT.add(tot, r)
    if not routed:
        NT.add(new, r)
    rows_out.append(NT.peak_record(r, routed_to_general=routed))
    print(NT.peak_line(r, 62), flush=True)
complete = all(row["general_ms"] is not None for row in rows_out)
ratio = tot["ours"] / tot["general"] if complete and tot["general"] > 0 else None
ratio_new = new["ours"] / new["general"] if complete and new["general"] > 0 else None
print(f"sum of the step's launches / the same layers on the general Conv3d f32 route: {ratio} (required <= 1.0); launches "
      f"that run csrc/conv2d_ae_f32.hip's own kernels only: {new['ours']:.3f} ms against {new['general']:.3f} ms = "
      f"{ratio_new}; rows marked [general route] are the general kernel's own time and fraction of peak")
print(NT.peak_total_line(62, tot))
print(json.dumps({"tool": "time_nb16", "batch": B, "image": S, "reps": REPS, "eager_ms": round(eager * 1e3, 4),
                  "graph_ms": round(replay * 1e3, 4), "samples_per_s_graph": round(B / replay, 1),
                  "step_gflop": round(tot["gflop"], 2), "step_of_peak_graph": round(tot["gflop"] / replay / 1e3 / NT.PEAK_TFLOPS, 4),
                  "launches_ours_ms": round(tot["ours"], 4), "launches_general_ms": round(tot["general"], 4),
                  "launches_torch_ms": round(tot["torch"], 4), "ours_over_general": round(ratio, 4) if ratio else None,
                  "new_kernels_ours_ms": round(new["ours"], 4), "new_kernels_general_ms": round(new["general"], 4),
                  "new_kernels_over_general": round(ratio_new, 4) if ratio_new else None, "calls_per_sample": INNER,
                  "launches": rows_out}))
if ratio is None or ratio > 1.0:
    sys.exit(f"time_nb16: the step's launches take {ratio} x the general Conv3d f32 route's time; the requirement is <= 1.0")
