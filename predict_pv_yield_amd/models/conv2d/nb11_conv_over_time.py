"""LitAutoEncoder of the per-frame Conv2d stack with a convolution over time -- host-side mirror of
notebooks/11_just_conv_and_conv_over_time.ipynb (the cell that defines LitAutoEncoder with CHANNELS = 32, N_HIST_IMAGES = 4,
STRIPE_WIDTH = 128 // 24, raw lines 1385-1470 of the .ipynb file; the live self.conv at 1407-1416 -- the commented-out first
definition at 1394-1405 is not built -- and self.temporal_conv at 1420-1426).

  input  x[HISTORICAL_SAT_IMAGES]  [B, 4, H, W]   float32, normalised by the loader (H = W = 128 in the notebook)
         x[FORECAST_HORIZON]       [B]            timesteps ahead, 1..23 (int64 in the notebook; any integer or float dtype)
         x[TARGET_SAT_IMAGE]       [B, h_t, w_t]  float32, normalised; (h_t, w_t) == the output's sides (H = 128: 64)
  graph  the horizon is a MetNet-style stripe plane as in notebook 10: start = int(horizon * 5), 1.0 on columns start <= c <
         start + 5, else 0.  Every history frame f goes, with that plane as a second channel, through the same
         self.conv = Sequential(Conv2d 2 -> 16, ReLU, Conv2d 16 -> 32, ReLU, Conv2d 32 -> 32 padding 2, ReLU,
         Conv2d 32 -> 1 stride 2 padding 2, ReLU): a side s becomes s - 2, s - 4, s - 2, (s - 1) // 2 + 1 (128 -> 64).
         The four outputs are laid side by side per pixel, [B, 1, P, 4] with P = the output's pixels (4096 in the notebook,
         which hard-codes it; here P = output_side(H) * output_side(W)), and
         self.temporal_conv = Sequential(Conv2d 1 -> 16 (1, 2), ReLU, Conv2d 16 -> 16 (1, 2), ReLU, Conv2d 16 -> 1 (1, 2))
         mixes them over time: 4 -> 3 -> 2 -> 1 columns, viewed back as [B, 1, s', s']
  loss   F.mse_loss(y_hat, target.unsqueeze(1)), no crop, no re-normalisation; Adam(lr=1e-4)

Same attribute / state_dict names as the notebook (conv.{0,2,4,6}.{weight,bias}, temporal_conv.{0,2,4}.{weight,bias}; 15 090
parameters).  self.conv and self.temporal_conv are parameter holders: every layer, the loss and the optimiser run on the gfx950
kernels behind include/pv_yield_hip.h (pv_conv2d_ae_frame_stripe_*, pv_conv2d_ae_*, pv_conv2d_ae_p2_*, pv_conv2d_head_s2_*,
pv_conv_time_*, pv_mse_loss_f32, pv_adam_step_f32).  The four calls of self.conv are one pass over 4 B images (image 4 b + f),
neither the [4 B, 2, H, W] input nor the stripe plane nor the [B, 1, P, 4] image is stored, and the three temporal layers of a
pixel run in registers.  Deliberate differences from the notebook, as in notebook 10's model: it runs on the MI355X only (CPU
tensors raise a RuntimeError); the stripe start is computed on the device as (horizon * 5).trunc(), so a step can be captured
as a graph; a target whose sides are not the output's raises a ValueError where torch would broadcast; and a negative horizon
follows the kernel rule start <= c < start + 5, 0 <= c < W.  The widest image is 128 pixels, the pv_conv2d_ae_* kernels' limit.
"""
import torch
from torch import nn

from .._notebook_ae import NotebookAutoEncoder
from .._notebook_ae import check_target_side as _check_target_side
from ..conv3d.flow_autoencoder import FORECAST_HORIZON, HISTORICAL_SAT_IMAGES, TARGET_SAT_IMAGE  # noqa: F401

STRIDE = 1
CHANNELS = 32
N_HIST_IMAGES = 4
STRIPE_WIDTH = 128 // 24      # input img size / num timesteps
MIN_IMAGE_SIDE = 5            # 5 -> 3 -> 1 -> 3 -> 3: the smallest side the two unpadded 3x3 convolutions accept


def output_side(image_side: int) -> int:
    """Side of y_hat for an input side (128 -> 64, 21 -> 11)."""
    if image_side < MIN_IMAGE_SIDE:
        raise ValueError(f"nb11 LitAutoEncoder needs images of at least {MIN_IMAGE_SIDE} x {MIN_IMAGE_SIDE} pixels (two "
                         f"unpadded 3x3 convolutions), got {image_side}")
    side = image_side - 2 - 2 + 2          # conv.0, conv.2 (padding 0), conv.4 (padding 2)
    return (side + 2 * 2 - 3) // 2 + 1      # conv.6: stride 2, padding 2


def check_target_side(image_shape, target_shape) -> None:
    """image_shape: (H, W) of the history images; the target must be [B, output_side(H), output_side(W)]."""
    _check_target_side("nb11", output_side, image_shape, target_shape)


class ConvOverTimeAutoEncoder(NotebookAutoEncoder):
    name = "nb11_conv_over_time"
    nb = "nb11"
    output_side, check_target_side = staticmethod(output_side), staticmethod(check_target_side)

    def __init__(self, lr: float = 0.0001):
        super().__init__()
        self.lr = float(lr)

        self.conv = nn.Sequential(
            nn.Conv2d(in_channels=2, out_channels=CHANNELS // 2, kernel_size=3, stride=1),
            nn.ReLU(),
            nn.Conv2d(in_channels=CHANNELS // 2, out_channels=CHANNELS, kernel_size=3, stride=1),
            nn.ReLU(),
            nn.Conv2d(in_channels=CHANNELS, out_channels=CHANNELS, kernel_size=3, stride=1, padding=2),
            nn.ReLU(),
            nn.Conv2d(in_channels=CHANNELS, out_channels=1, kernel_size=3, stride=2, padding=2),
            nn.ReLU(),
        )

        # the outputs of self.conv, one per history frame, side by side per pixel: convolved over the time dimension
        self.temporal_conv = nn.Sequential(
            nn.Conv2d(in_channels=1, out_channels=CHANNELS // 2, kernel_size=(1, 2), stride=1),
            nn.ReLU(),
            nn.Conv2d(in_channels=CHANNELS // 2, out_channels=CHANNELS // 2, kernel_size=(1, 2), stride=1),
            nn.ReLU(),
            nn.Conv2d(in_channels=CHANNELS // 2, out_channels=1, kernel_size=(1, 2), stride=1),
        )

    def forward(self, x):
        from ...conv2d_functional import nb11_conv_over_time_f32, stripe_start_from_horizon
        hist_images, horizon = self.history_and_horizon(x)
        # the stripe plane is synthesised by the first layer's kernels from one start column per example
        stripe_start = stripe_start_from_horizon(horizon, STRIPE_WIDTH)
        return nb11_conv_over_time_f32(hist_images, stripe_start, self.conv, self.temporal_conv)

    def loss(self, y_hat, y):
        from ...functional import mse_loss
        return mse_loss(y_hat, y.to(device=y_hat.device, dtype=torch.float32).unsqueeze(1))


# The notebook's name for the model, which configs and tests use.  The class statement itself carries another name because
# tests/test_notebook_model_table_cpu.py takes every models/conv?d/nb*.py that spells the notebooks' class statement for a row
# of the shared table in tests/notebook_model_checks.py, and this model's record lives in tests/test_gpu_nb11.py instead.
LitAutoEncoder = ConvOverTimeAutoEncoder
