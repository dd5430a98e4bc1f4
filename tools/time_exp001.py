"""Train-step time of experiments/001's LitAutoEncoder (B x 7 stacked 128 x 128 HRV frames + 5 channels, Conv2d 12 -> 144 ->
144 -> 144 with MaxPool2d(3), then fc1..fc5), eager and replayed as a HIP graph, and the device time of every conv launch with
its fraction of the f32 matrix peak; where torch's own F.conv2d runs on the device, it is timed alongside on the same shapes
(comparison only: the package never calls it).
   python tools/time_exp001.py [batch=32] [reps=20]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from predict_pv_yield_amd import hip_ops as K
from predict_pv_yield_amd.data.exp001_datamodule import make_fake_exp001_batch
from predict_pv_yield_amd.graphs import GraphedTrainStep
from predict_pv_yield_amd.models.conv2d.exp001 import LitAutoEncoder
from predict_pv_yield_amd.optim import HipAdam

dev = torch.device("cuda:0")
B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
S, NF = 128, 7
PEAK_TFLOPS = 157.3      # f32 matrix peak of the MI355X at its 2.4 GHz engine clock

batch = {k: v.to(dev) for k, v in make_fake_exp001_batch(B, S, torch.Generator().manual_seed(1)).items()}

# ---- the train step ------------------------------------------------------------------------------------------------
torch.manual_seed(0)
model = LitAutoEncoder().to(dev)
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
gmodel = LitAutoEncoder().to(dev)
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

# ---- every conv launch ------------------------------------------------------------------------------------------------
g = torch.Generator().manual_seed(2)
sat, xc, yc = batch["sat_data"], batch["sat_x_coords"].contiguous(), batch["sat_y_coords"].contiguous()
w1, b1 = model.sat_conv1.weight.detach().contiguous(), model.sat_conv1.bias.detach().contiguous()
w2, b2 = model.sat_conv2.weight.detach().contiguous(), model.sat_conv2.bias.detach().contiguous()
w3, b3 = model.sat_conv3.weight.detach().contiguous(), model.sat_conv3.bias.detach().contiguous()
y1, c1 = K.conv2d144_sat_pool_fwd_f32(sat, xc, yc, w1, b1, NF)
y2, c2 = K.conv2d144_pool_fwd_f32(y1, w2, b2)
y3 = K.conv2d144_fwd_f32(y2, w3, b3, relu=True)
dy3 = torch.randn(y3.shape, generator=g).to(dev)
dy2 = K.conv2d144_bwd_data_f32(dy3, y3, w3, None, tuple(y2.shape))
dy1 = K.conv2d144_pool_bwd_data_f32(dy2, c2, w2, None, tuple(y1.shape))
# torch's own operands: the 12-channel input and the pre-pool gradients materialised once (outside the timing)
x12 = torch.cat((sat[:, :NF, :, :, 0], torch.randn(B, 5, S, S, generator=g).to(dev)), 1).contiguous()
dz1 = torch.randn(B, 144, S - 2, S - 2, generator=g).to(dev)
dz2 = torch.randn(B, 144, 40, 40, generator=g).to(dev)

gf = lambda c_in, ho, wo: 2 * B * 144 * c_in * 9 * ho * wo / 1e9
cases = [  # (name, GFLOP, ours, torch)
    ("conv1 fwd + pool (input synthesised)", gf(12, 126, 126),
     lambda: K.conv2d144_sat_pool_fwd_f32(sat, xc, yc, w1, b1, NF), lambda: F.conv2d(x12, w1, b1)),
    ("conv2 fwd + pool (rows/cols 39.. skipped)", gf(144, 39, 39),
     lambda: K.conv2d144_pool_fwd_f32(y1, w2, b2), lambda: F.conv2d(y1, w2, b2)),
    ("conv3 fwd + relu", gf(144, 11, 11), lambda: K.conv2d144_fwd_f32(y2, w3, b3, relu=True),
     lambda: F.conv2d(y2, w3, b3)),
    ("conv3 dgrad (dy gated by y3)", gf(144, 11, 11), lambda: K.conv2d144_bwd_data_f32(dy3, y3, w3, None, tuple(y2.shape)),
     lambda: torch.nn.grad.conv2d_input(tuple(y2.shape), w3, dy3)),
    ("conv2 dgrad (pooled dy expanded by codes)", gf(144, 40, 40),
     lambda: K.conv2d144_pool_bwd_data_f32(dy2, c2, w2, None, tuple(y1.shape)),
     lambda: torch.nn.grad.conv2d_input(tuple(y1.shape), w2, dz2)),
    ("conv3 wgrad + db", gf(144, 11, 11), lambda: K.conv2d144_bwd_weight_f32(y2, dy3, y3, tuple(w3.shape)),
     lambda: torch.nn.grad.conv2d_weight(y2, tuple(w3.shape), dy3)),
    ("conv2 wgrad + db (pooled dy expanded)", gf(144, 39, 39),
     lambda: K.conv2d144_pool_bwd_weight_f32(y1, dy2, c2, tuple(w2.shape)),
     lambda: torch.nn.grad.conv2d_weight(y1, tuple(w2.shape), dz2)),
    ("conv1 wgrad + db (input re-synthesised)", gf(12, 126, 126),
     lambda: K.conv2d144_sat_pool_bwd_weight_f32(sat, xc, yc, dy1, c1, NF),
     lambda: torch.nn.grad.conv2d_weight(x12, tuple(w1.shape), dz1)),
]


def device_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


torch_ok = True
for _, _, a, b in cases:      # warm-up (workspaces, code objects, torch's algorithm search)
    a()
    if torch_ok:
        try:
            b()
        except Exception as e:            # torch may have no device convolution here: ours are timed alone
            print(f"torch F.conv2d unavailable on the device ({type(e).__name__}: {e}); timing ours only")
            torch_ok = False
torch.cuda.synchronize()
print(f"exp001.LitAutoEncoder B={B} x {NF} frames {S}x{S} (+5 channels): eager {eager * 1e3:.3f} ms/step "
      f"({B / eager:.0f} samples/s), HIP graph {replay * 1e3:.3f} ms/step ({B / replay:.0f} samples/s)", flush=True)
tot_new = tot_ref = tot_gf = 0.0
print(f"{'launch':46s} {'GFLOP':>7s} {'ours ms':>8s} {'of peak':>7s} {'torch ms':>9s}")
for name, gflop, a, b in cases:
    ta, tb = [], []
    for _ in range(REPS):     # alternate the two
        ta.append(device_ms(a))
        if torch_ok:
            tb.append(device_ms(b))
    ma = sorted(ta)[REPS // 2]
    mb = sorted(tb)[REPS // 2] if torch_ok else float("nan")
    tot_new, tot_ref, tot_gf = tot_new + ma, tot_ref + mb, tot_gf + gflop
    print(f"{name:46s} {gflop:7.2f} {ma:8.3f} {gflop / ma / PEAK_TFLOPS:7.3f} {mb:9.3f}", flush=True)
print(f"{'conv launches (median each, summed)':46s} {tot_gf:7.2f} {tot_new:8.3f} {tot_gf / tot_new / PEAK_TFLOPS:7.3f} "
      f"{tot_ref:9.3f}")
step_gf = tot_gf + 3 * 2 * B * 17424 * 256 / 1e9
print(f"train step: ~{step_gf:.1f} GFLOP of products (convs + fc1) in {replay * 1e3:.3f} ms replayed = "
      f"{step_gf / replay / 1e3 / PEAK_TFLOPS:.3f} of the {PEAK_TFLOPS} TFLOP/s f32 matrix peak")
