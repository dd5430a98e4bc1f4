"""torch.autograd.Function wrappers over the exact-f32 Conv2d 3x3 "valid" kernels: csrc/conv2d_f32.hip (experiments/002) and
the 144-channel kernels with fused MaxPool2d(3) of csrc/conv2d_pool_f32.hip (experiments/001) and the encoder / decoder
kernels of csrc/conv2d_ae_f32.hip (notebooks/16_maxpool.ipynb: Conv2d up to 128 wide, ConvTranspose2d, cropped MSE) and the
stride-2 Conv2d / ConvTranspose2d kernels of csrc/conv2d_s2_f32.hip (notebooks/14_back_to_2d_conv_AE.ipynb, 15_int16.ipynb) and
the padded 64 / 128-channel kernels, stripe first layer and stride-2 head of csrc/conv2d_wide_f32.hip (notebooks/10_just_conv.ipynb)
and the stride-2 64 / 128-channel Conv2d / ConvTranspose2d kernels, stride-2 stripe first layer, one-channel ConvTranspose2d
head and prediction-window MSE of csrc/conv2d_wide_s2_f32.hip (notebooks/09_horizon_represented_as_a_stripe.ipynb) and the
per-frame first layer and 128 -> 32 ConvTranspose2d of csrc/conv2d_frames_f32.hip (notebooks/07_multiple_historical_images.ipynb)
and the four-input first layer and stride-1 horizon ConvTranspose2d of csrc/conv2d_inputs_f32.hip
(notebooks/05_more_image_inputs.ipynb) and the per-frame stripe first layer and padded 32 -> 32 layer of csrc/conv2d_ae_f32.hip
with the convolution over time of csrc/conv_time_f32.hip (notebooks/11_just_conv_and_conv_over_time.ipynb).

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
  notebooks/07_multiple_historical_images.ipynb (raw lines of the .ipynb file)
    for each of the 4 history frames: self.encoder_conv(cat(hist_image, horizon plane)): Conv2d 2 -> 32 -> 32 -> 32, all
    stride 2, a ReLU after each; torch.cat(encoder_outs, dim=1)                                                :1364-1371, 1383-1394
    self.decoder_conv(encoder_outs): ConvTranspose2d 128 -> 32 -> 32 stride 2 with ReLU, ConvTranspose2d 32 -> 1 :1373-1379, 1396
    F.mse_loss(y_hat[:, :, :-1, :-1], y.unsqueeze(1))                                                          :1399-1402
  notebooks/05_more_image_inputs.ipynb (raw lines of the .ipynb file)
    self.encoder(cat(input_images, T0_IMAGES, optical_flow.squeeze())): Conv2d 4 -> 32 -> 32 -> 32, a ReLU after each :1356-1363, 1374-1380
    self.decoder(cat(embedding, forecast horizon plane)): ConvTranspose2d 33 -> 32 -> 32 with ReLU, ConvTranspose2d 32 -> 1
                                                                                                               :1365-1371, 1382-1387
    F.mse_loss(y_hat, y)                                                                                       :1394
  notebooks/11_just_conv_and_conv_over_time.ipynb (raw lines of the .ipynb file)
    for each of the 4 history frames: self.conv(cat(hist_img, forecast-horizon stripe plane)): Conv2d 2 -> 16 -> 32 -> 32
    (padding 2) -> 1 (stride 2, padding 2), a ReLU after each; conv_out.view((-1, 1, 4096, 1))                  :1407-1416, 1431-1447
    self.temporal_conv(torch.cat(conv_outs, dim=3)): Conv2d 1 -> 16 -> 16 -> 1, kernel (1, 2), ReLU between      :1420-1426, 1449-1451

Gating.  As in functional.Conv3dGeneralF32, the ReLU gating of an activation gradient is moved into the kernel that
produces it.  x_is_relu_output -> this layer's dx leaves already zeroed where x <= 0 (the lower layer's pre-activation
gradient).  dy_pregated -> the incoming dy was gated that way by the next layer, so backward reads it without touching y
again.  The two only pair up inside a chain, so the single-layer wrappers do not offer dy_pregated and no chain builder
passes either flag: conv_chain derives both from a layer's position, and states the rule.  The pooled layers return
relu(max_pool2d(z, 3)) (equal to max_pool2d(relu(z), 3)) and keep one byte per pooled output: the winning window position,
or "dead" where the maximum is <= 0.  Their backward expands the pooled gradient through those codes, which carry the ReLU
gate as well, so no gradient arriving at a pooled layer needs gating, and the layer above one leaves its dx ungated (the
pooled output is 0 exactly where its window is dead).

A new family: its record and one-line entry points in hip_ops.py, its *_OPS tuple and single-layer wrapper here, and a chain
builder that lists its model's layers for conv_chain.
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
# ... of the synthesised-input first layers, (forward, weight gradient): experiments/002's coordinate channels,
COORDS_OPS = (K.conv2d_coords_fwd_f32, K.conv2d_coords_bwd_weight_f32)
# the stripe plane at stride 1 (notebook 10) and stride 2 (notebook 09),
STRIPE_WIDE_OPS = (K.conv2d_wide_stripe_fwd_f32, K.conv2d_wide_stripe_bwd_weight_f32)
STRIPE_WIDE_S2_OPS = (K.conv2d_wide_s2_stripe_fwd_f32, K.conv2d_wide_s2_stripe_bwd_weight_f32)
# the raw counts of notebooks 14-16
COUNTS_AE_OPS = (K.conv2d_ae_counts_fwd_f32, K.conv2d_ae_counts_bwd_weight_f32)
COUNTS_S2_OPS = (K.conv2d_s2_counts_fwd_f32, K.conv2d_s2_counts_bwd_weight_f32)
# the per-frame history plane plus horizon plane of notebook 07 (and its 128 -> 32 ConvTranspose2d, a plain family)
FRAME_HORIZON_S2_OPS = (K.conv2d_s2_frame_horizon_fwd_f32, K.conv2d_s2_frame_horizon_bwd_weight_f32)
CONVT2D_S2_FRAMES_OPS = (K.convt2d_s2_frames_fwd_f32, K.convt2d_s2_frames_bwd_data_f32, K.convt2d_s2_frames_bwd_weight_f32)
# the flow prediction, t0 image and flow field of notebook 05, read in place as four channels
INPUTS_AE_OPS = (K.conv2d_ae_inputs_fwd_f32, K.conv2d_ae_inputs_bwd_weight_f32)
# notebook 11: the padded 32 -> 32 layer under the three-pass signatures (conv2d_ae_* with padding=2; hip_ops keeps one name
# per pass) and the per-frame history plane plus stripe plane


def _conv2d_ae_p2_fwd(x, weight, bias, relu=True):
    return K.conv2d_ae_fwd_f32(x, weight, bias, relu, padding=2)


def _conv2d_ae_p2_bwd_data(dy, dy_gate, weight, x_gate, x_shape):
    return K.conv2d_ae_bwd_data_f32(dy, dy_gate, weight, x_gate, x_shape, padding=2)


def _conv2d_ae_p2_bwd_weight(x, dy, dy_gate, weight_shape):
    return K.conv2d_ae_bwd_weight_f32(x, dy, dy_gate, weight_shape, padding=2)


CONV2D_AE_P2_OPS = (_conv2d_ae_p2_fwd, _conv2d_ae_p2_bwd_data, _conv2d_ae_p2_bwd_weight)
FRAME_STRIPE_AE_OPS = (K.conv2d_ae_frame_stripe_fwd_f32, K.conv2d_ae_frame_stripe_bwd_weight_f32)
# ... and of the conv with fused MaxPool2d(3): the forward returns (pooled, codes), the gradients take the codes
CONV2D144_POOL_OPS = (K.conv2d144_pool_fwd_f32, K.conv2d144_pool_bwd_data_f32, K.conv2d144_pool_bwd_weight_f32)
CONV2D_AE_POOL_OPS = (K.conv2d_ae_pool_fwd_f32, K.conv2d_ae_pool_bwd_data_f32, K.conv2d_ae_pool_bwd_weight_f32)
POOL_OPS = (CONV2D144_POOL_OPS, CONV2D_AE_POOL_OPS)


class SynthConvReLU(torch.autograd.Function):
    """A first layer whose input is synthesised inside its kernels (forward and weight gradient) from `inputs`, never stored:
    relu(conv(input built from inputs)).  ops = (forward, weight gradient): forward(*inputs, weight, bias, **scalars) and
    weight_gradient(*inputs, dy, weight_shape=..., **scalars).  No gradient flows to the inputs.
      COORDS_OPS                            sat [N, H, W, 12] channels-last, x_coords [N / t, W], y_coords [N / t, H]; t_per_example
      COUNTS_AE_OPS, COUNTS_S2_OPS          history [N, 4, H, W], flow prediction [N, H, W] (counts, int16 or f32), horizon [N] f32
      STRIPE_WIDE_OPS, STRIPE_WIDE_S2_OPS   history [N, n_hist, H, W] f32, stripe_start [N] int32 (the stripe plane is 1 on columns
                                            stripe_start[i] <= c < stripe_start[i] + stripe_width); stripe_width
      INPUTS_AE_OPS                         flow prediction [N, H, W], t0 image [N, H, W], flow field [N, 2, H, W], all f32: the four
                                            channels of notebook 05's x_cat
      FRAME_HORIZON_S2_OPS                  history [N, F, H, W] f32, horizon [N] f32: every frame with the horizon as a second,
                                            constant channel, the frames folded into the batch -> [N F, 32, ..]
      FRAME_STRIPE_AE_OPS                   history [N, F, H, W] f32, stripe_start [N] int32: every frame with the example's stripe
                                            plane as a second channel, the frames folded into the batch -> [N F, 16, ..]; stripe_width
      conv3d_wide_functional.HORIZON_WIDE_OPS   history [N, D, H, W] f32, horizon [N] f32 as a second, constant channel"""

    @staticmethod
    def forward(ctx, ops, inputs, weight, bias, scalars, dy_pregated):
        inputs = tuple(t.contiguous() for t in inputs)
        y = ops[0](*inputs, weight.contiguous(), bias.contiguous(), **scalars)
        ctx.save_for_backward(*inputs, None if dy_pregated else y)
        ctx.ops, ctx.scalars, ctx.weight_shape = ops, scalars, tuple(weight.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        *inputs, y = ctx.saved_tensors
        dy = dy.contiguous()
        if y is not None:
            dy = K.relu_gate_f32(dy, y)
        dw, db = ctx.ops[1](*inputs, dy, weight_shape=ctx.weight_shape, **ctx.scalars)
        return None, None, dw, db, None, None


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


def conv_chain(x, layers, last_relu):
    """A chain of fused conv (+ ReLU) layers in which every activation has exactly one consumer, the next layer.
    x: the first layer's input -- data or a pooled output, not a bare ReLU output -- or None where layers[0] synthesises its
    own.  layers, in order, each one of
      (ops, module)                     ConvReLU, or ConvPool where ops is one of POOL_OPS
      (ops, module, inputs[, scalars])  with x None: SynthConvReLU on the (forward, weight gradient) pair ops
      (Function, module, inputs)        a Function of one family that ends in a ReLU (or, as the last layer with last_relu False,
                                        in none), applied as (y, *inputs, weight, bias, x_is_relu_output, dy_pregated)
      a callable                        a view of the activation (squeeze, unsqueeze): the values, so the flags, stand
    Every layer but the last ends in a ReLU (the nn.ReLU modules of the notebooks' nn.Sequential are fused into the layers'
    kernels); the last one does where last_relu.

    The gating rule, which no caller spells out: layer i + 1's x_is_relu_output holds exactly when its input is a ReLU
    output and not a pooled one (the pool's codes carry that gate); layer i's dy_pregated holds exactly when it ends in such
    a ReLU and has a consumer in the chain, since that consumer then gates its data gradient by its input.  So no ReLU or
    mask kernel runs on its own, and the chain's own output, whose consumer is unknown, is gated by the layer itself."""
    y, gated = x, False                                 # gated: y is a ReLU output and not a pooled one
    for i, layer in enumerate(layers):
        if callable(layer):
            y = layer(y)
            continue
        ops, m, *extra = layer
        last = i == len(layers) - 1
        relu = last_relu or not last
        pooled = ops in POOL_OPS
        pregated = relu and not pooled and not last
        if y is None:
            y = SynthConvReLU.apply(ops, extra[0], m.weight, m.bias, extra[1] if len(extra) > 1 else {}, pregated)
        elif not isinstance(ops, tuple):
            y = ops.apply(y, *extra[0], m.weight, m.bias, gated, pregated)
        elif pooled:
            y = ConvPool.apply(ops, y, m.weight, m.bias, gated)
        else:
            y = ConvReLU.apply(ops, y, m.weight, m.bias, relu, gated, pregated)
        gated = relu and not pooled
    return y


def coords_conv2d_relu(sat, x_coords, y_coords, weight, bias, t_per_example):
    """relu(sat_conv1(17-channel input of experiments/002...py:180-208)); gradients to weight and bias only."""
    return SynthConvReLU.apply(COORDS_OPS, (sat, x_coords, y_coords), weight, bias, {"t_per_example": int(t_per_example)}, False)


def conv2d_relu(x, weight, bias, relu=True, x_is_relu_output=False):
    """nn.Conv2d(32, C_out, 3)(x) (+ ReLU).  x_is_relu_output: x is a ReLU output, so dx may leave gated by x > 0 (the lower
    layer's pre-activation gradient; the ReLU's own backward would zero those entries anyway)."""
    return ConvReLU.apply(CONV2D_OPS, x, weight, bias, bool(relu), bool(x_is_relu_output), False)


def sat_encoder_f32(sat, x_coords, y_coords, conv1, conv2, conv3, t_per_example):
    """relu(conv3(relu(conv2(relu(conv1(17-channel input)))))) of experiments/002...py:180-211; conv1..3 are nn.Conv2d."""
    first = (COORDS_OPS, conv1, (sat, x_coords, y_coords), {"t_per_example": int(t_per_example)})
    return conv_chain(None, [first, (CONV2D_OPS, conv2), (CONV2D_OPS, conv3)], last_relu=True)


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
    nn.Conv2d.  [B, 144, 11, 11] at 128 x 128.  conv3's output goes to fc1, whose data gradient is not gated."""
    y1 = SatConvPool.apply(sat, x_coords, y_coords, conv1.weight, conv1.bias, int(n_frames))
    return conv_chain(y1, [(CONV2D144_POOL_OPS, conv2), (CONV2D144_OPS, conv3)], last_relu=True)


# ---- notebooks/16_maxpool.ipynb ----------------------------------------------------------------------------------------
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


def _counts_inputs(history, flow_pred, horizon):
    return history, flow_pred, horizon.to(torch.float32)


def counts_conv_relu(history, flow_pred, horizon, weight, bias):
    """relu(encoder_conv1(normalised 6-channel input of 16_maxpool.ipynb:13760-13779)); gradients to weight and bias only."""
    return SynthConvReLU.apply(COUNTS_AE_OPS, _counts_inputs(history, flow_pred, horizon), weight, bias, {}, False)


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
    16_maxpool.ipynb:13760-13801; enc = the four nn.Conv2d, dec = the four nn.ConvTranspose2d."""
    return conv_chain(None, [(COUNTS_AE_OPS, enc[0], _counts_inputs(history, flow_pred, horizon)),
                             (CONV2D_AE_OPS, enc[1]), (CONV2D_AE_OPS, enc[2]), (CONV2D_AE_POOL_OPS, enc[3]),
                             *((CONVT2D_AE_OPS, m) for m in dec)], last_relu=False)


# ---- notebooks/14_back_to_2d_conv_AE.ipynb, 15_int16.ipynb -------------------------------------------------------------
def counts_conv_s2_relu(history, flow_pred, horizon, weight, bias):
    """relu(conv.0(normalised 6-channel input of 15_int16.ipynb:13766-13779)), stride 2; gradients to weight and bias only."""
    return SynthConvReLU.apply(COUNTS_S2_OPS, _counts_inputs(history, flow_pred, horizon), weight, bias, {}, False)


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
    8, 10, 12 nn.ConvTranspose2d, all stride 2)."""
    return conv_chain(None, [(COUNTS_S2_OPS, conv[0], _counts_inputs(history, flow_pred, horizon)),
                             *((CONV2D_S2_OPS, conv[i]) for i in (2, 4, 6)),
                             *((CONVT2D_S2_OPS, conv[i]) for i in (8, 10, 12))], last_relu=False)


# ---- notebooks/10_just_conv.ipynb ---------------------------------------------------------------------------------------
STRIPE_WIDTH = 128 // 24          # 10_just_conv.ipynb:1379: a constant, not derived from the image width


def stripe_start_from_horizon(horizon, stripe_width=STRIPE_WIDTH):
    """int(horizon[i] * stripe_width) of 10_just_conv.ipynb:1404 for every example at once, on the device (truncation toward
    zero, no host synchronisation, so a step can be captured as a graph).  Any integer or float dtype."""
    scaled = horizon * stripe_width
    return (scaled.trunc() if scaled.is_floating_point() else scaled).to(torch.int32)


def stripe_conv_relu(history, stripe_start, weight, bias, stripe_width=STRIPE_WIDTH):
    """relu(conv.0(cat(history, stripe plane))) of 10_just_conv.ipynb:1386-1387, 1398-1409; gradients to weight and bias only."""
    return SynthConvReLU.apply(STRIPE_WIDE_OPS, (history, stripe_start), weight, bias, {"stripe_width": int(stripe_width)}, False)


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
    2, 4, 6 nn.Conv2d)."""
    return conv_chain(None, [(STRIPE_WIDE_OPS, conv[0], (history, stripe_start), {"stripe_width": STRIPE_WIDTH}),
                             (CONV2D_WIDE_OPS, conv[2]), (CONV2D_WIDE_P2_OPS, conv[4]), (CONV2D_HEAD_S2_OPS, conv[6])],
                      last_relu=False)


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
    return SynthConvReLU.apply(STRIPE_WIDE_S2_OPS, (history, stripe_start), weight, bias, {"stripe_width": int(stripe_width)},
                               False)


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
    :1366-1398; encoder_conv / decoder_conv = the notebook's two nn.Sequential (modules 0, 2, 4 nn.Conv2d / nn.ConvTranspose2d)."""
    enc, dec = encoder_conv, decoder_conv
    return conv_chain(None, [(STRIPE_WIDE_S2_OPS, enc[0], (history, stripe_start), {"stripe_width": STRIPE_WIDTH}),
                             (CONV2D_WIDE_S2_OPS, enc[2]), (CONV2D_WIDE_S2_OPS, enc[4]),
                             (CONVT2D_WIDE_S2_OPS, dec[0]), (CONVT2D_WIDE_S2_OPS, dec[2]), (CONVT2D_HEAD_OPS, dec[4])],
                      last_relu=False)


# ---- notebooks/07_multiple_historical_images.ipynb -------------------------------------------------------------------------
def nb07_multi_hist_f32(history, horizon, encoder_conv, decoder_conv):
    """self.decoder_conv(cat([self.encoder_conv(cat(history[:, f:f + 1], horizon plane)) for f in range(4)], dim=1)) of
    07_multiple_historical_images.ipynb:1381-1396; encoder_conv / decoder_conv = the notebook's two nn.Sequential (modules 0,
    2, 4 nn.Conv2d / nn.ConvTranspose2d).  history [N, F, H, W], horizon [N] f32 -> [N, 1, 4 e + 5, 4 f + 5] for an encoder
    output of e x f.  The F calls of the encoder are one pass over F N images (image F i + f), so every encoder parameter's
    gradient is the sum over the frames, and the concatenation along the channels is the view [F N, 32, e, f] -> [N, F 32, e,
    f] of contiguous memory."""
    enc, dec = encoder_conv, decoder_conv
    n, frames = history.shape[:2]
    return conv_chain(None, [(FRAME_HORIZON_S2_OPS, enc[0], (history, horizon)), (CONV2D_S2_OPS, enc[2]), (CONV2D_S2_OPS, enc[4]),
                             lambda y: y.view(n, frames * y.shape[1], *y.shape[2:]),
                             (CONVT2D_S2_FRAMES_OPS, dec[0]), (CONVT2D_S2_OPS, dec[2]), (CONVT2D_HEAD_OPS, dec[4])],
                      last_relu=False)


# ---- notebooks/05_more_image_inputs.ipynb ----------------------------------------------------------------------------------
class HorizonConvTransposeS1ReLU(torch.autograd.Function):
    """First decoder layer of notebook 05: nn.ConvTranspose2d(33, 32, 3) (+ ReLU) on x [N, 32, H, W] f32 plus the forecast
    horizon [N] as a 33rd input channel, constant over the image, built inside the kernels (forward and weight gradient),
    never stored.  The horizon has no gradient; the 32 real channels' data gradient is the plain ConvTranspose2d's on the
    first 32 rows of the weight (contiguous, so a view).  The stride-1 twin of
    conv3d_wide_functional.HorizonConvTransposeReLU."""

    @staticmethod
    def forward(ctx, x, horizon, weight, bias, x_is_relu_output, dy_pregated):
        x, horizon = x.contiguous(), horizon.contiguous()
        y = K.convt2d_ae_horizon_fwd_f32(x, horizon, weight.contiguous(), bias.contiguous(), True)
        ctx.save_for_backward(x, horizon, weight, None if dy_pregated else y)
        ctx.x_is_relu_output = x_is_relu_output
        return y

    @staticmethod
    def backward(ctx, dy):
        x, horizon, weight, y = ctx.saved_tensors
        dy, weight = dy.contiguous(), weight.contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = K.convt2d_ae_bwd_data_f32(dy, y, weight[:K.CONVT_HORIZON_C], x if ctx.x_is_relu_output else None,
                                           tuple(x.shape))
        dw, db = K.convt2d_ae_horizon_bwd_weight_f32(x, horizon, dy, y, tuple(weight.shape))
        return dx, None, dw, db, None, None


def inputs_conv_relu(flow_pred, t0, flow_field, weight, bias):
    """relu(encoder.0(cat(input_images, T0_IMAGES, optical_flow))) of 05_more_image_inputs.ipynb:1357-1358, 1374-1380;
    gradients to weight and bias only."""
    return SynthConvReLU.apply(INPUTS_AE_OPS, (flow_pred, t0, flow_field), weight, bias, {}, False)


def horizon_conv_transpose_s1_relu(x, horizon, weight, bias, x_is_relu_output=False):
    """relu(decoder.0(cat(x, horizon plane))) of 05_more_image_inputs.ipynb:1366-1367, 1382-1387; no gradient to the horizon."""
    return HorizonConvTransposeS1ReLU.apply(x, horizon, weight, bias, bool(x_is_relu_output), False)


def nb05_more_inputs_f32(flow_pred, t0, flow_field, horizon, encoder, decoder):
    """self.decoder(cat(self.encoder(cat(input_images, T0_IMAGES, optical_flow)), horizon plane)) of
    05_more_image_inputs.ipynb:1373-1388; encoder / decoder = the notebook's two nn.Sequential (modules 0, 2, 4 nn.Conv2d /
    nn.ConvTranspose2d).  flow_pred and t0 [N, H, W], flow_field [N, 2, H, W], horizon [N], all f32 -> [N, 1, H, W]: the sides go
    down by 2 three times and up by 2 three times."""
    return conv_chain(None, [(INPUTS_AE_OPS, encoder[0], (flow_pred, t0, flow_field)),
                             (CONV2D_AE_OPS, encoder[2]), (CONV2D_AE_OPS, encoder[4]),
                             (HorizonConvTransposeS1ReLU, decoder[0], (horizon,)),
                             (CONVT2D_AE_OPS, decoder[2]), (CONVT2D_HEAD_OPS, decoder[4])], last_relu=False)


# ---- notebooks/11_just_conv_and_conv_over_time.ipynb ------------------------------------------------------------------------
class ConvOverTime(torch.autograd.Function):
    """self.temporal_conv of notebook 11 on the per-frame stack's output u [4 N, 1, H, W] (image 4 i + f): three (1, 2)
    convolutions over the four frame values of each pixel, ReLU between, in registers -> [N, 1, H, W].  Saves u and the
    parameters; backward recomputes the hidden layers and returns du and the six parameter gradients from one launch.
    Argument order as conv_chain applies a Function: the activation, the first two layers' parameters, then the last
    layer's weight and bias and the two flags.  x_is_relu_output: du leaves gated by u > 0, the pre-activation gradient of
    the layer that made u (pv_conv2d_head_s2_* take no dy_gate).  No ReLU follows the last layer, so dy is never pregated."""

    @staticmethod
    def forward(ctx, u, w1, b1, w2, b2, w3, b3, x_is_relu_output, dy_pregated):
        assert not dy_pregated, "no ReLU follows temporal_conv: it is a chain's last layer, with last_relu False"
        tensors = tuple(t.contiguous() for t in (u, w1, b1, w2, b2, w3, b3))
        ctx.save_for_backward(*tensors[:-1])
        ctx.x_is_relu_output = x_is_relu_output
        return K.conv_time_fwd_f32(*tensors)

    @staticmethod
    def backward(ctx, dy):
        u, *params = ctx.saved_tensors
        return K.conv_time_bwd_f32(u, dy.contiguous(), *params, ctx.x_is_relu_output) + (None, None)


def conv_over_time(u, temporal_conv, x_is_relu_output=False):
    """temporal_conv(cat of the four frames' outputs along a new last axis) of 11_just_conv_and_conv_over_time.ipynb:1446-1451;
    temporal_conv = the notebook's nn.Sequential (modules 0, 2, 4 nn.Conv2d with kernel (1, 2)).  x_is_relu_output: du leaves
    gated by u > 0."""
    t = temporal_conv
    return ConvOverTime.apply(u, t[0].weight, t[0].bias, t[2].weight, t[2].bias, t[4].weight, t[4].bias,
                              bool(x_is_relu_output), False)


def nb11_layers(history, stripe_start, conv, temporal_conv):
    """Notebook 11 as conv_chain's layer table: the per-frame stack, every layer of it ending in a ReLU, then the convolution
    over time as the chain's last layer, which ends in none (last_relu=False).  The head's ReLU gate is applied to du by the
    convolution over time, so the head receives its dy pregated like the layers below it."""
    t = temporal_conv
    return [(FRAME_STRIPE_AE_OPS, conv[0], (history, stripe_start), {"stripe_width": STRIPE_WIDTH}),
            (CONV2D_AE_OPS, conv[2]), (CONV2D_AE_P2_OPS, conv[4]), (CONV2D_HEAD_S2_OPS, conv[6]),
            (ConvOverTime, t[4], (t[0].weight, t[0].bias, t[2].weight, t[2].bias))]


def nb11_conv_over_time_f32(history, stripe_start, conv, temporal_conv):
    """self.temporal_conv(cat([self.conv(cat(history[:, f:f + 1], stripe plane)).view(-1, 1, P, 1) for f in range(4)], dim=3))
    .view(-1, 1, s', s') of 11_just_conv_and_conv_over_time.ipynb:1428-1451; conv / temporal_conv = the notebook's two
    nn.Sequential.  history [N, 4, H, W], stripe_start [N] int32 -> [N, 1, s', s'].  The four calls of self.conv are one pass
    over 4 N images (image 4 i + f), so every parameter's gradient is the sum over the frames, and the [N, 1, P, 4] image is
    the head's output [4 N, 1, s', s'] read in place."""
    return conv_chain(None, nb11_layers(history, stripe_start, conv, temporal_conv), last_relu=False)
