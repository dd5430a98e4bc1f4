"""torch.autograd.Function wrappers over the exact-f32 Conv2d 3x3 "valid" kernels: csrc/conv2d_f32.hip (experiments/002) and
the 144-channel kernels with fused MaxPool2d(3) of csrc/conv2d_pool_f32.hip (experiments/001) and the encoder / decoder
kernels of csrc/conv2d_ae_f32.hip (notebooks/16_maxpool.ipynb: Conv2d up to 128 wide, ConvTranspose2d, cropped MSE) and the
stride-2 Conv2d / ConvTranspose2d kernels of csrc/conv2d_s2_f32.hip (notebooks/14_back_to_2d_conv_AE.ipynb, 15_int16.ipynb) and
the padded 64 / 128-channel kernels, stripe first layer and stride-2 head of csrc/conv2d_wide_f32.hip (notebooks/10_just_conv.ipynb)
and the stride-2 64 / 128-channel Conv2d / ConvTranspose2d kernels, stride-2 stripe first layer, one-channel ConvTranspose2d
head and prediction-window MSE of csrc/conv2d_wide_s2_f32.hip (notebooks/09_horizon_represented_as_a_stripe.ipynb).

Reference operators replaced:
  experiments/002_cnn_processes_single_sat_image_then_rnn.py
    F.relu(self.sat_conv1(torch.cat((sat_data, center_marker, x_coords, y_coords, pixel_x, pixel_y), dim=1)))  :180-209
    F.relu(self.sat_conv2(out)), F.relu(self.sat_conv3(out))                                                  :210-211
  experiments/001_CNN_concat_all_timesteps_as_channels.py
    self.maxpool(F.relu(self.sat_conv1(torch.cat((frames, center_marker, x_coords, ...), dim=1))))             :264-307
    self.maxpool(F.relu(self.sat_conv2(out)))                                                                 :308-309
    F.relu(self.sat_conv3(out))                                                                               :310
  notebooks/16_maxpool.ipynb (raw lines of the .ipynb file)
    F.relu(self.encoder_conv1(cat(normalise_images_in_model(cat(history, flow)), horizon plane)))             :13760-13779
    F.relu(self.encoder_conv2(out)), F.relu(self.encoder_conv3(out))                                          :13782-13785
    self.maxpool(F.relu(self.encoder_conv4(out)))                                                             :13788-13789
    F.relu(self.decoder_conv1..3(out)), self.decoder_conv4(out)                                               :13793-13801
    F.mse_loss(y_hat.squeeze(), normalise_images_in_model(y)[..., 8:-8, 8:-8])                                :13805-13809
  notebooks/15_int16.ipynb (raw lines of the .ipynb file; notebook 14 has the same stack)
    self.conv(cat(normalise_images_in_model(cat(history, flow)), horizon plane)): nn.Sequential of Conv2d 6 -> 16 -> 32 -> 32
    -> 32 and ConvTranspose2d 32 -> 32 -> 16 -> 1, all 3x3 stride 2, ReLU between                              :13746-13780
    F.mse_loss(y_hat.squeeze(), normalise_images_in_model(y)[..., :-1, :-1])                                  :13783-13788
  notebooks/10_just_conv.ipynb (raw lines of the .ipynb file)
    self.conv(cat(hist_images, forecast-horizon stripe plane)): nn.Sequential of Conv2d 5 -> 64 -> 128 -> 128 (padding 2) and
    Conv2d 128 -> 1 (stride 2, padding 2), ReLU between                                                        :1386-1410
  notebooks/09_horizon_represented_as_a_stripe.ipynb (raw lines of the .ipynb file)
    self.encoder_conv(cat(hist_images, forecast-horizon stripe plane)): Conv2d 5 -> 64 -> 128 -> 128, all stride 2, a
    ReLU after each                                                                                            :1366-1370, 1382-1397
    self.decoder_conv(out): ConvTranspose2d 128 -> 128 -> 128 stride 2 with ReLU, ConvTranspose2d 128 -> 1     :1375-1379
    F.mse_loss(y_hat[:, :, :-1, :-1], y.unsqueeze(1))                                                          :1402-1403

Gating.  As in functional.Conv3dGeneralF32, the ReLU gating of an activation gradient is moved into the kernel that
produces it.  x_is_relu_output -> this layer's dx leaves already zeroed where x <= 0 (the lower layer's pre-activation
gradient).  In the unpooled chain, dy_pregated -> the incoming dy was gated that way by the next layer, so backward reads it
without touching y again; it is set only inside sat_encoder_f32, where that pairing holds by construction.  The pooled
layers return relu(max_pool2d(z, 3)) (equal to max_pool2d(relu(z), 3)) and keep one byte per pooled output: the winning
window position, or "dead" where the maximum is <= 0.  Their backward expands the pooled gradient through those codes,
which carry the ReLU gate as well, so no gradient arriving at a pooled layer needs gating; above a pooled layer the
x_is_relu_output gate equals the codes' (the pooled output is 0 exactly where its window is dead), so sat_encoder001_f32
leaves it off.  Its one ReLU output without a pool, conv3's, goes to fc1, whose data gradient is not gated, so conv3 gates
its own dy by its output.
"""
import torch

from . import hip_ops as K

# entry points of the plain (unpooled) conv: (forward, data gradient, weight gradient); each is a one-line call into the one
# implementation of its pass in hip_ops.py, with the family's record (a new family is added there, then named here)
CONV2D_OPS = (K.conv2d_fwd_f32, K.conv2d_bwd_data_f32, K.conv2d_bwd_weight_f32)
CONV2D144_OPS = (K.conv2d144_fwd_f32, K.conv2d144_bwd_data_f32, K.conv2d144_bwd_weight_f32)
CONV2D_AE_OPS = (K.conv2d_ae_fwd_f32, K.conv2d_ae_bwd_data_f32, K.conv2d_ae_bwd_weight_f32)
CONVT2D_AE_OPS = (K.convt2d_ae_fwd_f32, K.convt2d_ae_bwd_data_f32, K.convt2d_ae_bwd_weight_f32)
CONV2D_S2_OPS = (K.conv2d_s2_fwd_f32, K.conv2d_s2_bwd_data_f32, K.conv2d_s2_bwd_weight_f32)
CONVT2D_S2_OPS = (K.convt2d_s2_fwd_f32, K.convt2d_s2_bwd_data_f32, K.convt2d_s2_bwd_weight_f32)
# notebook 10: the padded wide family (one tuple per padding) and the stride-2 one-channel head
CONV2D_WIDE_OPS = (K.conv2d_wide_fwd_f32, K.conv2d_wide_bwd_data_f32, K.conv2d_wide_bwd_weight_f32)
CONV2D_WIDE_P2_OPS = (K.conv2d_wide_p2_fwd_f32, K.conv2d_wide_p2_bwd_data_f32, K.conv2d_wide_p2_bwd_weight_f32)
CONV2D_HEAD_S2_OPS = (K.conv2d_head_s2_fwd_f32, K.conv2d_head_s2_bwd_data_f32, K.conv2d_head_s2_bwd_weight_f32)
# notebook 09: the stride-2 wide layers and the one-output-channel ConvTranspose2d head
CONV2D_WIDE_S2_OPS = (K.conv2d_wide_s2_fwd_f32, K.conv2d_wide_s2_bwd_data_f32, K.conv2d_wide_s2_bwd_weight_f32)
CONVT2D_WIDE_S2_OPS = (K.convt2d_wide_s2_fwd_f32, K.convt2d_wide_s2_bwd_data_f32, K.convt2d_wide_s2_bwd_weight_f32)
CONVT2D_HEAD_OPS = (K.convt2d_head_fwd_f32, K.convt2d_head_bwd_data_f32, K.convt2d_head_bwd_weight_f32)
# ... of the stripe first layer: (forward, weight gradient), stride 1 (notebook 10) and stride 2 (notebook 09)
STRIPE_WIDE_OPS = (K.conv2d_wide_stripe_fwd_f32, K.conv2d_wide_stripe_bwd_weight_f32)
STRIPE_WIDE_S2_OPS = (K.conv2d_wide_s2_stripe_fwd_f32, K.conv2d_wide_s2_stripe_bwd_weight_f32)
# ... of the raw-counts first layer: (forward, weight gradient)
COUNTS_AE_OPS = (K.conv2d_ae_counts_fwd_f32, K.conv2d_ae_counts_bwd_weight_f32)
COUNTS_S2_OPS = (K.conv2d_s2_counts_fwd_f32, K.conv2d_s2_counts_bwd_weight_f32)
# ... and of the conv with fused MaxPool2d(3): the forward returns (pooled, codes), the gradients take the codes
CONV2D144_POOL_OPS = (K.conv2d144_pool_fwd_f32, K.conv2d144_pool_bwd_data_f32, K.conv2d144_pool_bwd_weight_f32)
CONV2D_AE_POOL_OPS = (K.conv2d_ae_pool_fwd_f32, K.conv2d_ae_pool_bwd_data_f32, K.conv2d_ae_pool_bwd_weight_f32)


class CoordsConv2dReLU(torch.autograd.Function):
    """First layer: sat [N, H, W, 12] channels-last, x_coords [N / t, W], y_coords [N / t, H]; the 17-channel input is
    synthesised inside the kernels (forward and weight gradient), never stored.  No gradient flows to the inputs."""

    @staticmethod
    def forward(ctx, sat, x_coords, y_coords, weight, bias, t_per_example, dy_pregated):
        sat, x_coords, y_coords = sat.contiguous(), x_coords.contiguous(), y_coords.contiguous()
        y = K.conv2d_coords_fwd_f32(sat, x_coords, y_coords, weight.contiguous(), bias.contiguous(), t_per_example)
        ctx.save_for_backward(sat, x_coords, y_coords, None if dy_pregated else y)
        ctx.t_per_example, ctx.weight_shape = t_per_example, tuple(weight.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        sat, x_coords, y_coords, y = ctx.saved_tensors
        dy = dy.contiguous()
        if y is not None:
            dy = K.relu_gate_f32(dy, y)
        dw, db = K.conv2d_coords_bwd_weight_f32(sat, x_coords, y_coords, dy, ctx.t_per_example, ctx.weight_shape)
        return None, None, None, dw, db, None, None


class ConvReLU(torch.autograd.Function):
    """nn.Conv2d(C_in, C_out, 3) (+ ReLU) on NCHW f32 through one family of entry points, ops = CONV2D_OPS (32 -> 32 or 4),
    CONV2D144_OPS (144 -> 144) or CONV2D_AE_OPS (16 or 32 -> 32, planes up to 128 wide); with CONVT2D_AE_OPS,
    nn.ConvTranspose2d(C_in, C_out, 3) for (C_in, C_out) = (32, 32), (32, 16), (16, 16), (16, 1); CONV2D_S2_OPS and
    CONVT2D_S2_OPS are the stride-2 layers of notebooks 14 / 15 ((16 or 32) -> 32; (32, 32), (32, 16), (16, 1)).  Saves the
    input, and the output only where backward gates dy by it (relu and not dy_pregated)."""

    @staticmethod
    def forward(ctx, ops, x, weight, bias, relu, x_is_relu_output, dy_pregated):
        x = x.contiguous()
        y = ops[0](x, weight.contiguous(), bias.contiguous() if bias is not None else None, relu)
        ctx.save_for_backward(x, weight, y if (relu and not dy_pregated) else None)
        ctx.ops, ctx.has_bias, ctx.x_is_relu_output = ops, bias is not None, x_is_relu_output
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        _, bwd_data, bwd_weight = ctx.ops
        dy, weight = dy.contiguous(), weight.contiguous()
        dx = None
        if ctx.needs_input_grad[1]:
            dx = bwd_data(dy, y, weight, x if ctx.x_is_relu_output else None, tuple(x.shape))
        dw, db = bwd_weight(x, dy, y, tuple(weight.shape))
        return None, dx, dw, (db if ctx.has_bias else None), None, None, None


class SatConvPool(torch.autograd.Function):
    """First layer of experiments/001: sat [B, T, H, W, 1], frames 0..n_frames-1 stacked as channels plus five synthesised
    channels, built inside the kernels (forward and weight gradient), never stored.  No gradient flows to the inputs."""

    @staticmethod
    def forward(ctx, sat, x_coords, y_coords, weight, bias, n_frames):
        sat, x_coords, y_coords = sat.contiguous(), x_coords.contiguous(), y_coords.contiguous()
        y, codes = K.conv2d144_sat_pool_fwd_f32(sat, x_coords, y_coords, weight.contiguous(), bias.contiguous(), n_frames)
        ctx.save_for_backward(sat, x_coords, y_coords, codes)
        ctx.n_frames = n_frames
        return y

    @staticmethod
    def backward(ctx, dy):
        sat, x_coords, y_coords, codes = ctx.saved_tensors
        dw, db = K.conv2d144_sat_pool_bwd_weight_f32(sat, x_coords, y_coords, dy.contiguous(), codes, ctx.n_frames)
        return None, None, None, dw, db, None


class ConvPool(torch.autograd.Function):
    """relu(max_pool2d(nn.Conv2d(C, C, 3)(x), 3)) on NCHW f32, ops = CONV2D144_POOL_OPS (C = 144) or CONV2D_AE_POOL_OPS (C =
    32, planes up to 128 wide); saves the input and the codes."""

    @staticmethod
    def forward(ctx, ops, x, weight, bias, x_is_relu_output):
        x = x.contiguous()
        y, codes = ops[0](x, weight.contiguous(), bias.contiguous())
        ctx.save_for_backward(x, weight, codes)
        ctx.ops, ctx.x_is_relu_output = ops, x_is_relu_output
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, codes = ctx.saved_tensors
        _, bwd_data, bwd_weight = ctx.ops
        dy, weight = dy.contiguous(), weight.contiguous()
        dx = None
        if ctx.needs_input_grad[1]:
            dx = bwd_data(dy, codes, weight, x if ctx.x_is_relu_output else None, tuple(x.shape))
        dw, db = bwd_weight(x, dy, codes, tuple(weight.shape))
        return None, dx, dw, db, None


def coords_conv2d_relu(sat, x_coords, y_coords, weight, bias, t_per_example):
    """relu(sat_conv1(17-channel input of experiments/002...py:180-208)); gradients to weight and bias only."""
    return CoordsConv2dReLU.apply(sat, x_coords, y_coords, weight, bias, int(t_per_example), False)


def conv2d_relu(x, weight, bias, relu=True, x_is_relu_output=False):
    """nn.Conv2d(32, C_out, 3)(x) (+ ReLU).  x_is_relu_output: x is a ReLU output, so dx may leave gated by x > 0 (the lower
    layer's pre-activation gradient; the ReLU's own backward would zero those entries anyway)."""
    return ConvReLU.apply(CONV2D_OPS, x, weight, bias, bool(relu), bool(x_is_relu_output), False)


def sat_encoder_f32(sat, x_coords, y_coords, conv1, conv2, conv3, t_per_example):
    """relu(conv3(relu(conv2(relu(conv1(17-channel input)))))) of experiments/002...py:180-211; conv1..3 are nn.Conv2d.
    The two inner activations have exactly one consumer each, the next layer's conv, whose data gradient leaves gated by
    them (x_is_relu_output): so their producers skip gating the arriving gradient again (dy_pregated).  That pairing is
    only valid inside this chain, which is why the flag is not offered by coords_conv2d_relu / conv2d_relu."""
    y1 = CoordsConv2dReLU.apply(sat, x_coords, y_coords, conv1.weight, conv1.bias, int(t_per_example), True)
    y2 = ConvReLU.apply(CONV2D_OPS, y1, conv2.weight, conv2.bias, True, True, True)
    return ConvReLU.apply(CONV2D_OPS, y2, conv3.weight, conv3.bias, True, True, False)


def sat_conv_pool_f32(sat, x_coords, y_coords, weight, bias, n_frames):
    """maxpool(relu(sat_conv1(stacked frames + 5 channels))) of experiments/001...py:264-307; gradients to weight and bias
    only."""
    return SatConvPool.apply(sat, x_coords, y_coords, weight, bias, int(n_frames))


def conv_pool_f32(x, weight, bias, x_is_relu_output=False):
    """maxpool(relu(nn.Conv2d(144, 144, 3)(x))).  x_is_relu_output: dx leaves gated by x > 0."""
    return ConvPool.apply(CONV2D144_POOL_OPS, x, weight, bias, bool(x_is_relu_output))


def conv144_relu(x, weight, bias, relu=True, x_is_relu_output=False):
    """nn.Conv2d(144, 144, 3)(x) (+ ReLU).  x_is_relu_output: dx leaves gated by x > 0."""
    return ConvReLU.apply(CONV2D144_OPS, x, weight, bias, bool(relu), bool(x_is_relu_output), False)


def sat_encoder001_f32(sat, x_coords, y_coords, conv1, conv2, conv3, n_frames):
    """relu(conv3(pool(relu(conv2(pool(relu(conv1(stacked input)))))))) of experiments/001...py:264-310; conv1..3 are
    nn.Conv2d.  [B, 144, 11, 11] at 128 x 128.  conv2 and conv3 read pooled outputs, whose layers route the gradient through
    their codes, so their dx is not gated again."""
    y1 = SatConvPool.apply(sat, x_coords, y_coords, conv1.weight, conv1.bias, int(n_frames))
    y2 = ConvPool.apply(CONV2D144_POOL_OPS, y1, conv2.weight, conv2.bias, False)
    return ConvReLU.apply(CONV2D144_OPS, y2, conv3.weight, conv3.bias, True, False, False)


# ---- notebooks/16_maxpool.ipynb ----------------------------------------------------------------------------------------
class CountsConvReLU(torch.autograd.Function):
    """First layer of notebooks 14-16: history [N, 4, H, W] and flow prediction [N, H, W] as raw counts (int16 or f32),
    horizon [N]; the normalised 6-channel input is built inside the kernels (forward and weight gradient), never stored.
    ops = COUNTS_AE_OPS (stride 1, notebook 16) or COUNTS_S2_OPS (stride 2).  No gradient flows to the inputs."""

    @staticmethod
    def forward(ctx, ops, history, flow_pred, horizon, weight, bias, dy_pregated):
        history, flow_pred = history.contiguous(), flow_pred.contiguous()
        horizon = horizon.to(torch.float32).contiguous()
        y = ops[0](history, flow_pred, horizon, weight.contiguous(), bias.contiguous())
        ctx.save_for_backward(history, flow_pred, horizon, None if dy_pregated else y)
        ctx.ops, ctx.weight_shape = ops, tuple(weight.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        history, flow_pred, horizon, y = ctx.saved_tensors
        dy = dy.contiguous()
        if y is not None:
            dy = K.relu_gate_f32(dy, y)
        dw, db = ctx.ops[1](history, flow_pred, horizon, dy, ctx.weight_shape)
        return None, None, None, None, dw, db, None


class MseNorm(torch.autograd.Function):
    """F.mse_loss(y_hat, normalise(target)[window]): y_hat [N, P, Q] f32, target raw counts; the gradient 2 (y_hat - y) / count
    is produced in the same pass.  window None: target [N, P + 16, Q + 16] and the crop [..., 8:-8, 8:-8], whose entry point
    checks that the sides match; (row0, col0): target [N, T, U] and [..., row0:row0 + P, col0:col0 + Q]."""

    @staticmethod
    def forward(ctx, y_hat, target, window):
        y_hat, target = y_hat.contiguous(), target.contiguous()
        if window is None:
            out, grad = K.mse_crop_norm_f32(y_hat, target, need_grad=True)
        else:
            out, grad = K.mse_window_norm_f32(y_hat, target, *window, need_grad=True)
        ctx.save_for_backward(grad)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None


def counts_conv_relu(history, flow_pred, horizon, weight, bias):
    """relu(encoder_conv1(normalised 6-channel input of 16_maxpool.ipynb:13760-13779)); gradients to weight and bias only."""
    return CountsConvReLU.apply(COUNTS_AE_OPS, history, flow_pred, horizon, weight, bias, False)


def conv2d_ae_relu(x, weight, bias, relu=True, x_is_relu_output=False):
    """nn.Conv2d(16 or 32, 32, 3)(x) (+ ReLU), planes up to 128 wide.  x_is_relu_output: dx leaves gated by x > 0."""
    return ConvReLU.apply(CONV2D_AE_OPS, x, weight, bias, bool(relu), bool(x_is_relu_output), False)


def conv_relu_pool32(x, weight, bias, x_is_relu_output=False):
    """maxpool(relu(nn.Conv2d(32, 32, 3)(x))).  x_is_relu_output: dx leaves gated by x > 0."""
    return ConvPool.apply(CONV2D_AE_POOL_OPS, x, weight, bias, bool(x_is_relu_output))


def conv_transpose2d_relu(x, weight, bias, relu=True, x_is_relu_output=False):
    """nn.ConvTranspose2d(C_in, C_out, 3)(x) (+ ReLU).  x_is_relu_output: dx leaves gated by x > 0."""
    return ConvReLU.apply(CONVT2D_AE_OPS, x, weight, bias, bool(relu), bool(x_is_relu_output), False)


def mse_crop_norm(y_hat, target):
    """F.mse_loss(y_hat, normalise_images_in_model(target)[..., 8:-8, 8:-8]) of 16_maxpool.ipynb:13805-13809."""
    return MseNorm.apply(y_hat, target, None)


def nb16_autoencoder_f32(history, flow_pred, horizon, enc, dec):
    """decoder_conv4(relu(decoder_conv3(... maxpool(relu(encoder_conv4(... relu(encoder_conv1(input))))))) of
    16_maxpool.ipynb:13760-13801; enc = the four nn.Conv2d, dec = the four nn.ConvTranspose2d.  Every inner ReLU output has
    one consumer, the next layer, whose data gradient leaves gated by it (x_is_relu_output), so its producer skips gating
    the arriving gradient (dy_pregated).  The pooled output is 0 exactly where its window is dead, which the codes carry,
    so decoder_conv1 leaves its dx ungated.  The pairing only holds inside this chain."""
    y = CountsConvReLU.apply(COUNTS_AE_OPS, history, flow_pred, horizon, enc[0].weight, enc[0].bias, True)
    y = ConvReLU.apply(CONV2D_AE_OPS, y, enc[1].weight, enc[1].bias, True, True, True)
    y = ConvReLU.apply(CONV2D_AE_OPS, y, enc[2].weight, enc[2].bias, True, True, True)
    y = ConvPool.apply(CONV2D_AE_POOL_OPS, y, enc[3].weight, enc[3].bias, True)
    y = ConvReLU.apply(CONVT2D_AE_OPS, y, dec[0].weight, dec[0].bias, True, False, True)
    y = ConvReLU.apply(CONVT2D_AE_OPS, y, dec[1].weight, dec[1].bias, True, True, True)
    y = ConvReLU.apply(CONVT2D_AE_OPS, y, dec[2].weight, dec[2].bias, True, True, True)
    return ConvReLU.apply(CONVT2D_AE_OPS, y, dec[3].weight, dec[3].bias, False, True, False)


# ---- notebooks/14_back_to_2d_conv_AE.ipynb, 15_int16.ipynb -------------------------------------------------------------
def counts_conv_s2_relu(history, flow_pred, horizon, weight, bias):
    """relu(conv.0(normalised 6-channel input of 15_int16.ipynb:13766-13779)), stride 2; gradients to weight and bias only."""
    return CountsConvReLU.apply(COUNTS_S2_OPS, history, flow_pred, horizon, weight, bias, False)


def conv2d_s2_relu(x, weight, bias, relu=True, x_is_relu_output=False):
    """nn.Conv2d(16 or 32, 32, 3, stride=2)(x) (+ ReLU), planes up to 128 wide.  x_is_relu_output: dx leaves gated by x > 0."""
    return ConvReLU.apply(CONV2D_S2_OPS, x, weight, bias, bool(relu), bool(x_is_relu_output), False)


def conv_transpose2d_s2_relu(x, weight, bias, relu=True, x_is_relu_output=False):
    """nn.ConvTranspose2d(C_in, C_out, 3, stride=2)(x) (+ ReLU).  x_is_relu_output: dx leaves gated by x > 0."""
    return ConvReLU.apply(CONVT2D_S2_OPS, x, weight, bias, bool(relu), bool(x_is_relu_output), False)


def mse_window_norm(y_hat, target, row0=0, col0=0):
    """F.mse_loss(y_hat, normalise_images_in_model(target)[..., row0:row0 + P, col0:col0 + Q]); (0, 0) with a target one
    larger than y_hat is y[..., :-1, :-1] of 15_int16.ipynb:13783-13788."""
    return MseNorm.apply(y_hat, target, (int(row0), int(col0)))


def nb15_autoencoder_f32(history, flow_pred, horizon, conv):
    """self.conv(images) of 15_int16.ipynb:13746-13780; conv = the notebook's nn.Sequential (modules 0, 2, 4, 6 nn.Conv2d and
    8, 10, 12 nn.ConvTranspose2d, all stride 2; the nn.ReLU modules between them are fused into the layers' kernels).  Every
    inner ReLU output has one consumer, the next layer, whose data gradient leaves gated by it (x_is_relu_output), so its
    producer skips gating the arriving gradient (dy_pregated): no ReLU or mask kernel runs on its own.  The pairing only
    holds inside this chain."""
    y = CountsConvReLU.apply(COUNTS_S2_OPS, history, flow_pred, horizon, conv[0].weight, conv[0].bias, True)
    for i in (2, 4, 6):
        y = ConvReLU.apply(CONV2D_S2_OPS, y, conv[i].weight, conv[i].bias, True, True, True)
    for i in (8, 10):
        y = ConvReLU.apply(CONVT2D_S2_OPS, y, conv[i].weight, conv[i].bias, True, True, True)
    return ConvReLU.apply(CONVT2D_S2_OPS, y, conv[12].weight, conv[12].bias, False, True, False)


# ---- notebooks/10_just_conv.ipynb ---------------------------------------------------------------------------------------
STRIPE_WIDTH = 128 // 24          # 10_just_conv.ipynb:1379: a constant, not derived from the image width


class StripeConvReLU(torch.autograd.Function):
    """First layer of notebooks 09 and 10: history [N, n_hist, H, W] f32 plus the forecast-horizon stripe plane (1 on columns
    stripe_start[i] <= c < stripe_start[i] + stripe_width), built inside the kernels (forward and weight gradient), never
    stored.  ops = STRIPE_WIDE_OPS (stride 1, notebook 10) or STRIPE_WIDE_S2_OPS (stride 2, notebook 09).  No gradient flows
    to the inputs."""

    @staticmethod
    def forward(ctx, ops, history, stripe_start, weight, bias, stripe_width, dy_pregated):
        history, stripe_start = history.contiguous(), stripe_start.contiguous()
        y = ops[0](history, stripe_start, weight.contiguous(), bias.contiguous(), stripe_width)
        ctx.save_for_backward(history, stripe_start, None if dy_pregated else y)
        ctx.ops, ctx.stripe_width, ctx.weight_shape = ops, stripe_width, tuple(weight.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        history, stripe_start, y = ctx.saved_tensors
        dy = dy.contiguous()
        if y is not None:
            dy = K.relu_gate_f32(dy, y)
        dw, db = ctx.ops[1](history, stripe_start, dy, ctx.weight_shape, ctx.stripe_width)
        return None, None, None, dw, db, None, None


def stripe_start_from_horizon(horizon, stripe_width=STRIPE_WIDTH):
    """int(horizon[i] * stripe_width) of 10_just_conv.ipynb:1404 for every example at once, on the device (truncation toward
    zero, no host synchronisation, so a step can be captured as a graph).  Any integer or float dtype."""
    scaled = horizon * stripe_width
    return (scaled.trunc() if scaled.is_floating_point() else scaled).to(torch.int32)


def stripe_conv_relu(history, stripe_start, weight, bias, stripe_width=STRIPE_WIDTH):
    """relu(conv.0(cat(history, stripe plane))) of 10_just_conv.ipynb:1386-1387, 1398-1409; gradients to weight and bias only."""
    return StripeConvReLU.apply(STRIPE_WIDE_OPS, history, stripe_start, weight, bias, int(stripe_width), False)


def conv2d_wide_relu(x, weight, bias, relu=True, x_is_relu_output=False, padding=0):
    """nn.Conv2d(64 or 128, 128, 3, padding=0 or 2)(x) (+ ReLU), planes up to 128 wide.  x_is_relu_output: dx leaves gated by
    x > 0."""
    ops = {0: CONV2D_WIDE_OPS, 2: CONV2D_WIDE_P2_OPS}[int(padding)]
    return ConvReLU.apply(ops, x, weight, bias, bool(relu), bool(x_is_relu_output), False)


def conv2d_head_s2(x, weight, bias, x_is_relu_output=False):
    """nn.Conv2d(C_in, 1, 3, stride=2, padding=2)(x), no ReLU.  x_is_relu_output: dx leaves gated by x > 0."""
    return ConvReLU.apply(CONV2D_HEAD_S2_OPS, x, weight, bias, False, bool(x_is_relu_output), False)


def nb10_just_conv_f32(history, stripe_start, conv):
    """self.conv(cat(hist_images, stripe plane)) of 10_just_conv.ipynb:1386-1410; conv = the notebook's nn.Sequential (modules 0,
    2, 4, 6 nn.Conv2d; the nn.ReLU modules between them are fused into the layers' kernels).  Every inner ReLU output has one
    consumer, the next layer, whose data gradient leaves gated by it (x_is_relu_output), so its producer skips gating the
    arriving gradient (dy_pregated): no ReLU or mask kernel runs on its own.  The pairing only holds inside this chain."""
    y = StripeConvReLU.apply(STRIPE_WIDE_OPS, history, stripe_start, conv[0].weight, conv[0].bias, STRIPE_WIDTH, True)
    y = ConvReLU.apply(CONV2D_WIDE_OPS, y, conv[2].weight, conv[2].bias, True, True, True)
    y = ConvReLU.apply(CONV2D_WIDE_P2_OPS, y, conv[4].weight, conv[4].bias, True, True, True)
    return ConvReLU.apply(CONV2D_HEAD_S2_OPS, y, conv[6].weight, conv[6].bias, False, True, False)


# ---- notebooks/09_horizon_represented_as_a_stripe.ipynb ------------------------------------------------------------------
class MsePredWindow(torch.autograd.Function):
    """F.mse_loss(y_hat[..., row0:row0 + T, col0:col0 + U], target): y_hat [N, P, Q] and target [N, T, U] f32; the gradient,
    2 (y_hat - y) / count inside the window and exactly 0 outside, is produced in the same pass."""

    @staticmethod
    def forward(ctx, y_hat, target, row0, col0):
        out, grad = K.mse_pred_window_f32(y_hat.contiguous(), target.contiguous(), row0, col0, need_grad=True)
        ctx.save_for_backward(grad)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None, None


def stripe_conv_s2_relu(history, stripe_start, weight, bias, stripe_width=STRIPE_WIDTH):
    """relu(encoder_conv.0(cat(history, stripe plane))) of 09_horizon_represented_as_a_stripe.ipynb:1366-1367, 1382-1397,
    stride 2; gradients to weight and bias only."""
    return StripeConvReLU.apply(STRIPE_WIDE_S2_OPS, history, stripe_start, weight, bias, int(stripe_width), False)


def conv2d_wide_s2_relu(x, weight, bias, relu=True, x_is_relu_output=False):
    """nn.Conv2d(64 or 128, 128, 3, stride=2)(x) (+ ReLU), planes up to 128 wide.  x_is_relu_output: dx leaves gated by x > 0."""
    return ConvReLU.apply(CONV2D_WIDE_S2_OPS, x, weight, bias, bool(relu), bool(x_is_relu_output), False)


def conv_transpose2d_wide_s2_relu(x, weight, bias, relu=True, x_is_relu_output=False):
    """nn.ConvTranspose2d(128, 128, 3, stride=2)(x) (+ ReLU).  x_is_relu_output: dx leaves gated by x > 0."""
    return ConvReLU.apply(CONVT2D_WIDE_S2_OPS, x, weight, bias, bool(relu), bool(x_is_relu_output), False)


def conv_transpose2d_head(x, weight, bias, x_is_relu_output=False):
    """nn.ConvTranspose2d(C_in, 1, 3)(x), no ReLU.  x_is_relu_output: dx leaves gated by x > 0."""
    return ConvReLU.apply(CONVT2D_HEAD_OPS, x, weight, bias, False, bool(x_is_relu_output), False)


def mse_pred_window(y_hat, target, row0=0, col0=0):
    """F.mse_loss(y_hat[..., row0:row0 + T, col0:col0 + U], target); (0, 0) with a target one smaller than y_hat is
    F.mse_loss(y_hat[:, :, :-1, :-1], y.unsqueeze(1)) of 09_horizon_represented_as_a_stripe.ipynb:1402-1403."""
    return MsePredWindow.apply(y_hat, target, int(row0), int(col0))


def nb09_stripe_ae_f32(history, stripe_start, encoder_conv, decoder_conv):
    """self.decoder_conv(self.encoder_conv(cat(hist_images, stripe plane))) of 09_horizon_represented_as_a_stripe.ipynb
    :1366-1398; encoder_conv / decoder_conv = the notebook's two nn.Sequential (modules 0, 2, 4 nn.Conv2d / nn.ConvTranspose2d;
    the nn.ReLU modules between them are fused into the layers' kernels).  Every inner ReLU output has one consumer, the next
    layer, whose data gradient leaves gated by it (x_is_relu_output), so its producer skips gating the arriving gradient
    (dy_pregated): no ReLU or mask kernel runs on its own.  The pairing only holds inside this chain."""
    enc, dec = encoder_conv, decoder_conv
    y = StripeConvReLU.apply(STRIPE_WIDE_S2_OPS, history, stripe_start, enc[0].weight, enc[0].bias, STRIPE_WIDTH, True)
    for i in (2, 4):
        y = ConvReLU.apply(CONV2D_WIDE_S2_OPS, y, enc[i].weight, enc[i].bias, True, True, True)
    for i in (0, 2):
        y = ConvReLU.apply(CONVT2D_WIDE_S2_OPS, y, dec[i].weight, dec[i].bias, True, True, True)
    return ConvReLU.apply(CONVT2D_HEAD_OPS, y, dec[4].weight, dec[4].bias, False, True, False)
