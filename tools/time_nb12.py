"""Train-step time of notebooks/12_just_3d_conv.ipynb's LitAutoEncoder (B x 4 x 128 x 128 normalised frames plus the horizon
channel, Conv3d 2 -> 64 -> 128 -> 128 -> 128 -> 1 with kernel (2, 3, 3)), eager and replayed as a HIP graph, and the device time
of every conv launch of the step with its fraction of the f32 matrix peak.  Alongside, in the same process and on the same
device: torch's own conv3d kernels (comparison only: the package never calls them; the first layer's two-channel input is
materialised outside the timing), and the yardstick the new kernels are held to.  The general Conv3d f32 route refuses every
64 / 128-channel launch of this model (its weight tile exceeds the LDS), so the like-for-like yardstick is the 2-D kernel
these were derived from: pv_conv2d_wide_{fwd,bwd_data,bwd_weight}_f32 at 128 -> 128, padding 2, on the same B x 128 x 128
planes.  Each 128 -> 128 pass of the new family is reported as the ratio of its FLOP rate to that pass's.
FLOPs: `gflop` counts every tap of the kernel as torch would (the issue's figures); `gflop_run` leaves out the depth taps that
fall on depth padding, which the kernels skip, and is what the rates and ratios use.
Warm-up first, device-side event timing of INNER back-to-back calls per sample, the median of REPS alternating samples (ours,
torch, ours, ...), inputs resident before the timed region; the samples' min and max are kept as the spread.  Prints a table
and one JSON line.
   python tools/time_nb12.py [batch=64] [reps=7]"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
import nb_timing as NT
from predict_pv_yield_amd import hip_ops as K
from predict_pv_yield_amd.models.conv3d.nb12_just_3d_conv import LitAutoEncoder, output_side

dev = torch.device("cuda:0")
B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
S = 128
T = output_side(S)
INNER = 2                # back-to-back calls per event pair

g = torch.Generator().manual_seed(1)
batch = {"HISTORICAL_SAT_IMAGES": torch.randn(B, 4, S, S, generator=g).to(dev),
         "FORECAST_HORIZON": ((torch.randint(1, 25, (B,), generator=g).float() - 12.5) / 6.9222).to(dev),
         "TARGET_SAT_IMAGE": torch.randn(B, T, T, generator=g).to(dev)}

# ---- the train step, eager and replayed (tools/nb_timing.py) ----------------------------------------------------------
model, eager, replay = NT.graph_and_eager(LitAutoEncoder, batch, 0.0001, REPS, warmup=2)
print(NT.step_line("nb12", B, S, eager, replay), flush=True)

# ---- every conv launch of the step -------------------------------------------------------------------------------------
hist, horizon = batch["HISTORICAL_SAT_IMAGES"], batch["FORECAST_HORIZON"]
P = lambda i: (model.conv[i].weight.detach().contiguous(), model.conv[i].bias.detach().contiguous())      # noqa: E731
(w0, b0), (w2, b2), (w4, b4), (w6, b6), (w8, b8) = (P(i) for i in (0, 2, 4, 6, 8))
y0 = K.conv3d_wide_horizon_fwd_f32(hist, horizon, w0, b0)
y2 = K.conv3d_wide_fwd_f32(y0, w2, b2, padding=(0, 1, 1))
y4 = K.conv3d_wide_fwd_f32(y2, w4, b4, padding=(1, 1, 1))
y6 = K.conv3d_wide_fwd_f32(y4, w6, b6, padding=(0, 1, 1))
y8 = K.conv3d_head_d2_fwd_f32(y6, w8, b8)
rnd = lambda t: torch.randn(t.shape, generator=g).to(dev)      # noqa: E731
dy8, dy6, dy4, dy2, dy0 = (rnd(t) for t in (y8, y6, y4, y2, y0))
x0 = torch.cat((hist.unsqueeze(1), horizon.view(-1, 1, 1, 1, 1).expand(B, 1, 4, S, S)), 1).contiguous()


def real_taps(d_in, pd):
    """Fraction of the (output slice, depth tap) pairs whose source slice exists."""
    d_out = d_in + 2 * pd - 1
    pairs = [(d, kd) for d in range(d_out) for kd in (0, 1) if 0 <= d + kd - pd < d_in]
    return len(pairs) / (2 * d_out)


def conv_rows(name, x, w, b, dy, pad, stride, ours_fwd, ours_dgrad, ours_wgrad, first=False):
    """(name, GFLOP, GFLOP run, ours, torch) of one Conv3d layer's launches."""
    n, ci, d = x.shape[:3]
    co = w.shape[0]
    gf = 2 * n * co * ci * 18 * dy.shape[2] * dy.shape[3] * dy.shape[4] / 1e9
    run = gf * real_taps(d, pad[0])
    rows = [(f"{name} fwd", gf, run, ours_fwd, lambda: F.conv3d(x, w, b, stride=stride, padding=pad))]
    if not first:
        rows.append((f"{name} dgrad", gf, run, ours_dgrad,
                     lambda: torch.nn.grad.conv3d_input(tuple(x.shape), w, dy, stride=stride, padding=pad)))
    rows.append((f"{name} wgrad + db", gf, run, ours_wgrad,
                 lambda: torch.nn.grad.conv3d_weight(x, tuple(w.shape), dy, stride=stride, padding=pad)))
    return rows


cases = []
cases += conv_rows("conv.0 2->64 (horizon synthesised while staged)", x0, w0, b0, dy0, (0, 1, 1), 1,
                   lambda: K.conv3d_wide_horizon_fwd_f32(hist, horizon, w0, b0), None,
                   lambda: K.conv3d_wide_horizon_bwd_weight_f32(hist, horizon, dy0, tuple(w0.shape)), first=True)
for nm, x, w, b, dy, pd in (("conv.2 64->128 pd0", y0, w2, b2, dy2, 0), ("conv.4 128->128 pd1", y2, w4, b4, dy4, 1),
                            ("conv.6 128->128 pd0", y4, w6, b6, dy6, 0)):
    pad = (pd, 1, 1)
    cases += conv_rows(nm, x, w, b, dy, pad, 1,
                       lambda x=x, w=w, b=b, pad=pad: K.conv3d_wide_fwd_f32(x, w, b, padding=pad),
                       lambda x=x, w=w, dy=dy, pad=pad: K.conv3d_wide_bwd_data_f32(dy, None, w, x, tuple(x.shape), padding=pad),
                       lambda x=x, w=w, dy=dy, pad=pad: K.conv3d_wide_bwd_weight_f32(x, dy, None, tuple(w.shape), padding=pad))
cases += conv_rows("conv.8 128->1 s2 (head on the depth-2 view)", y6, w8, b8, dy8, (0, 1, 1), (1, 2, 2),
                   lambda: K.conv3d_head_d2_fwd_f32(y6, w8, b8),
                   lambda: K.conv3d_head_d2_bwd_data_f32(dy8, None, w8, y6, tuple(y6.shape)),
                   lambda: K.conv3d_head_d2_bwd_weight_f32(y6, dy8, None, tuple(w8.shape)))

# the yardstick: the parent's 2-D kernels at 128 -> 128, padding 2, on B x 128 x 128 planes
xs = torch.randn(B, 128, S, S, generator=g).to(dev)
ws, bs = torch.randn(128, 128, 3, 3, generator=g).to(dev) * (9 * 128) ** -0.5, torch.zeros(128, device=dev)
ys = K.conv2d_wide_fwd_f32(xs, ws, bs, padding=2)
dys = rnd(ys)
gf_y = 2 * B * 128 * 128 * 9 * ys.shape[2] * ys.shape[3] / 1e9
yard = [("conv2d_wide 128->128 p2 fwd", gf_y, gf_y, lambda: K.conv2d_wide_fwd_f32(xs, ws, bs, padding=2), None),
        ("conv2d_wide 128->128 p2 dgrad", gf_y, gf_y,
         lambda: K.conv2d_wide_bwd_data_f32(dys, None, ws, xs, tuple(xs.shape), padding=2), None),
        ("conv2d_wide 128->128 p2 wgrad + db", gf_y, gf_y,
         lambda: K.conv2d_wide_bwd_weight_f32(xs, dys, None, tuple(ws.shape), padding=2), None)]


rows_out, rate = [], {}
tot = {"ours": 0.0, "torch": 0.0, "gflop": 0.0, "run": 0.0}
run_of = {name: run for name, _, run, _, _ in cases + yard}
in_step = {name for name, *_ in cases}
print(f"{'launch':50s} {'GFLOP':>8s} {'run':>8s} {'ours ms':>8s} {'spread':>15s} {'of peak':>7s} {'torch ms':>9s}")
# two routes here, ours and torch in turn: there is no general route for these layers
for r in NT.time_cases([(name, gflop, ours, None, torch_fn) for name, gflop, _, ours, torch_fn in cases + yard], REPS, INNER, warmup=2):
    run = run_of[r.name]
    rate[r.name] = run / r.ours.med      # GFLOP / ms = TFLOP/s
    if r.name in in_step:
        tot["ours"] += r.ours.med
        tot["torch"] += r.torch.med if r.torch else 0.0
        tot["gflop"] += r.gflop
        tot["run"] += run
    rows_out.append({"launch": r.name, "gflop": round(r.gflop, 3), "gflop_run": round(run, 3), "ours_ms": round(r.ours.med, 4),
                     "ours_ms_min": round(r.ours.lo, 4), "ours_ms_max": round(r.ours.hi, 4),
                     "of_peak": round(run / r.ours.med / NT.PEAK_TFLOPS, 4), "torch_ms": NT.r4(r.torch.med)})
    print(f"{r.name:50s} {r.gflop:8.2f} {run:8.2f} {r.ours.med:8.3f} {NT.spread(r.ours)} {run / r.ours.med / NT.PEAK_TFLOPS:7.3f} "
          f"{r.torch.med:9.3f}", flush=True)

ratios = {}
for layer in ("conv.4 128->128 pd1", "conv.6 128->128 pd0"):
    for p in ("fwd", "dgrad", "wgrad + db"):
        ratios[f"{layer} {p}"] = round(rate[f"{layer} {p}"] / rate[f"conv2d_wide 128->128 p2 {p}"], 4)
print("FLOP rate of each new 128 -> 128 pass over the same pass of conv2d_wide 128 -> 128 p2:", ratios)
print(f"{'conv launches of a step (median each, summed)':50s} {tot['gflop']:8.2f} {tot['run']:8.2f} {tot['ours']:8.3f} "
      f"{'':15s} {tot['run'] / tot['ours'] / NT.PEAK_TFLOPS:7.3f} {tot['torch']:9.3f}")
print(json.dumps({"tool": "time_nb12", "batch": B, "image": S, "reps": REPS, "calls_per_sample": INNER,
                  "eager_ms": round(eager * 1e3, 4), "graph_ms": round(replay * 1e3, 4),
                  "samples_per_s_graph": round(B / replay, 2), "step_gflop": round(tot["gflop"], 2),
                  "step_gflop_run": round(tot["run"], 2),
                  "step_of_peak_graph": round(tot["run"] / replay / 1e3 / NT.PEAK_TFLOPS, 4),
                  "launches_ours_ms": round(tot["ours"], 4), "launches_torch_ms": round(tot["torch"], 4),
                  "rate_over_conv2d_wide_128_p2": ratios, "launches": rows_out}))
