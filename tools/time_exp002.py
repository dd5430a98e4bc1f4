"""Train-step time of experiments/002's LitModel (B x 19 images of 32 x 32 x 12, Conv2d 17 -> 32 -> 32 -> 4, then GRUs), eager
and replayed as a HIP graph, and the device time of every Conv2d launch against the general Conv3d f32 route
(pv_conv3d_general_*_f32 as a 1x3x3 conv with T = 1) on the same shapes, alternating in one process.
   python tools/time_exp002.py [batch=32] [reps=20]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from predict_pv_yield_amd import hip_ops as K
from predict_pv_yield_amd.data.exp002_datamodule import make_fake_exp002_batch
from predict_pv_yield_amd.graphs import GraphedTrainStep
from predict_pv_yield_amd.models.conv2d.exp002 import LitModel
from predict_pv_yield_amd.optim import HipAdam

dev = torch.device("cuda:0")
B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
T, S = 19, 32
N = B * T
PEAK_TFLOPS = 157.3      # f32 matrix (= f32 vector) peak of the MI355X at its 2.4 GHz engine clock

batch = {k: v.to(dev) for k, v in make_fake_exp002_batch(B, S, torch.Generator().manual_seed(1)).items()}

# ---- the train step ------------------------------------------------------------------------------------------------
torch.manual_seed(0)
model = LitModel().to(dev)
opt = model.configure_optimizers()


def step():
    opt.zero_grad(set_to_none=True)
    model.training_step(batch, 0).backward()
    opt.step()


for _ in range(3):
    step()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(REPS):
    step()
torch.cuda.synchronize()
eager = (time.perf_counter() - t0) / REPS

torch.manual_seed(0)
gmodel = LitModel().to(dev)
gopt = HipAdam(gmodel.parameters(), lr=0.001, capturable=True)
graphed = GraphedTrainStep(gmodel, gopt, batch, warmup=3)
for _ in range(3):
    graphed(batch)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(REPS):
    graphed(batch)
torch.cuda.synchronize()
replay = (time.perf_counter() - t0) / REPS
graphed.close()
print(f"exp002.LitModel B={B} x {T} images {S}x{S}x12: eager {eager * 1e3:.3f} ms/step ({B / eager:.0f} samples/s), "
      f"HIP graph {replay * 1e3:.3f} ms/step ({B / replay:.0f} samples/s)", flush=True)

# ---- every conv launch against the general route ----------------------------------------------------------------------
g = torch.Generator().manual_seed(2)
sat = batch["sat_data"].reshape(N, S, S, 12).contiguous()
xc, yc = batch["sat_x_coords"].contiguous(), batch["sat_y_coords"].contiguous()
w1, b1 = model.sat_conv1.weight.detach().contiguous(), model.sat_conv1.bias.detach().contiguous()
w2, b2 = model.sat_conv2.weight.detach().contiguous(), model.sat_conv2.bias.detach().contiguous()
w3, b3 = model.sat_conv3.weight.detach().contiguous(), model.sat_conv3.bias.detach().contiguous()
y1 = K.conv2d_coords_fwd_f32(sat, xc, yc, w1, b1, T)
y2 = K.conv2d_fwd_f32(y1, w2, b2, relu=True)
y3 = K.conv2d_fwd_f32(y2, w3, b3, relu=True)
dy3 = torch.randn(y3.shape, generator=g).to(dev)
dy2 = K.conv2d_bwd_data_f32(dy3, y3, w3, y2, tuple(y2.shape))
dy1 = K.conv2d_bwd_data_f32(dy2, None, w2, y1, tuple(y1.shape))
# the general route's operands: NCDHW views with T = 1, the 17-channel input materialised once (outside the timing)
from predict_pv_yield_amd.models.conv2d.exp002 import SAT_X_MEAN, SAT_X_STD, SAT_Y_MEAN, SAT_Y_STD
pix = (torch.arange(S, device=dev) - 64) / 37
x17 = torch.cat((sat.permute(0, 3, 1, 2),
                 torch.zeros(N, 1, S, S, device=dev).index_fill_(2, torch.arange(S // 2 - 2, S // 2 + 2, device=dev), 1)
                 * torch.zeros(N, 1, S, S, device=dev).index_fill_(3, torch.arange(S // 2 - 2, S // 2 + 2, device=dev), 1),
                 ((xc - SAT_X_MEAN) / SAT_X_STD)[:, None, None, :].expand(-1, 1, S, -1).repeat_interleave(T, 0),
                 ((yc - SAT_Y_MEAN) / SAT_Y_STD)[:, None, :, None].expand(-1, 1, -1, S).repeat_interleave(T, 0),
                 pix[None, None, None, :].expand(N, 1, S, S), pix[None, None, :, None].expand(N, 1, S, S)), 1).contiguous()
v = lambda t: t.unsqueeze(2)          # [N, C, H, W] -> [N, C, 1, H, W]
wv = lambda w: w.unsqueeze(2)

cases = [  # (name, GFLOP, new, general)
    ("conv1 fwd (17->32, input assembled)", 2 * N * 32 * 17 * 9 * 30 * 30 / 1e9,
     lambda: K.conv2d_coords_fwd_f32(sat, xc, yc, w1, b1, T),
     lambda: K.conv3d_general_fwd_f32(v(x17), wv(w1), b1, relu=True)),
    ("conv2 fwd (32->32)", 2 * N * 32 * 32 * 9 * 28 * 28 / 1e9,
     lambda: K.conv2d_fwd_f32(y1, w2, b2, relu=True), lambda: K.conv3d_general_fwd_f32(v(y1), wv(w2), b2, relu=True)),
    ("conv3 fwd (32->4)", 2 * N * 4 * 32 * 9 * 26 * 26 / 1e9,
     lambda: K.conv2d_fwd_f32(y2, w3, b3, relu=True), lambda: K.conv3d_general_fwd_f32(v(y2), wv(w3), b3, relu=True)),
    ("conv3 dgrad (gated by y3, y2)", 2 * N * 4 * 32 * 9 * 26 * 26 / 1e9,
     lambda: K.conv2d_bwd_data_f32(dy3, y3, w3, y2, tuple(y2.shape)),
     lambda: K.conv3d_general_bwd_data_f32(v(dy3), v(y3), wv(w3), (N, 32, 1, 28, 28), x_mask=v(y2))),
    ("conv2 dgrad (gated by y1)", 2 * N * 32 * 32 * 9 * 28 * 28 / 1e9,
     lambda: K.conv2d_bwd_data_f32(dy2, None, w2, y1, tuple(y1.shape)),
     lambda: K.conv3d_general_bwd_data_f32(v(dy2), None, wv(w2), (N, 32, 1, 30, 30), x_mask=v(y1))),
    ("conv3 wgrad + db (delegates to the general kernel)", 2 * N * 4 * 32 * 9 * 26 * 26 / 1e9,
     lambda: K.conv2d_bwd_weight_f32(y2, dy3, y3, (4, 32, 3, 3)),
     lambda: K.conv3d_general_bwd_weight_f32(v(y2), v(dy3), v(y3), (4, 32, 1, 3, 3))),
    ("conv2 wgrad + db", 2 * N * 32 * 32 * 9 * 28 * 28 / 1e9,
     lambda: K.conv2d_bwd_weight_f32(y1, dy2, None, (32, 32, 3, 3)),
     lambda: K.conv3d_general_bwd_weight_f32(v(y1), v(dy2), None, (32, 32, 1, 3, 3))),
    ("conv1 wgrad + db (input re-synthesised)", 2 * N * 32 * 17 * 9 * 30 * 30 / 1e9,
     lambda: K.conv2d_coords_bwd_weight_f32(sat, xc, yc, dy1, T, (32, 17, 3, 3)),
     lambda: K.conv3d_general_bwd_weight_f32(v(x17), v(dy1), None, (32, 17, 1, 3, 3))),
]


def device_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


for _, _, a, b in cases:      # warm-up (workspaces, code objects)
    a(), b()
torch.cuda.synchronize()
tot_new = tot_gen = tot_gf = 0.0
print(f"{'launch':50s} {'GFLOP':>7s} {'new ms':>8s} {'general ms':>10s} {'speed-up':>8s} {'new TF/s':>8s}")
for name, gf, a, b in cases:
    ta, tb = [], []
    for _ in range(REPS):     # alternate the two routes
        ta.append(device_ms(a))
        tb.append(device_ms(b))
    ma, mb = sorted(ta)[REPS // 2], sorted(tb)[REPS // 2]
    tot_new, tot_gen, tot_gf = tot_new + ma, tot_gen + mb, tot_gf + gf
    print(f"{name:50s} {gf:7.2f} {ma:8.3f} {mb:10.3f} {mb / ma:7.2f}x {gf / ma:8.1f}", flush=True)
print(f"{'conv family (median per launch, summed)':50s} {tot_gf:7.2f} {tot_new:8.3f} {tot_gen:10.3f} {tot_gen / tot_new:7.2f}x "
      f"{tot_gf / tot_new:8.1f}")
print(f"conv family: {tot_gf / tot_new / PEAK_TFLOPS * 100:.1f} % of the {PEAK_TFLOPS} TFLOP/s f32 matrix peak "
      f"(general route {tot_gf / tot_gen / PEAK_TFLOPS * 100:.1f} %)")
