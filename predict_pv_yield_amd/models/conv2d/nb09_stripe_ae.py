"""LitAutoEncoder of the stride-2 stripe autoencoder -- host-side mirror of notebooks/09_horizon_represented_as_a_stripe.ipynb
(the cell that defines LitAutoEncoder with STRIDE = 2, CHANNELS = 128, N_HIST_IMAGES = 4, STRIPE_WIDTH = 128 // 24, raw lines
1356-1416 of the .ipynb file; encoder_conv at 1366-1370, decoder_conv at 1375-1379).  Notebook 10 was cut down from it.

  input  x[HISTORICAL_SAT_IMAGES]  [B, 4, H, W]   float32, normalised by the loader (H = W = 128 in the notebook)
         x[FORECAST_HORIZON]       [B]            timesteps ahead, 1..23 (int64 in the notebook; any integer or float dtype)
         x[TARGET_SAT_IMAGE]       [B, h_t, w_t]  float32, normalised; (h_t, w_t) == the output's sides - 1 (H = 128: 64)
  graph  a fifth input plane carries the horizon as a MetNet-style stripe: start = int(horizon * 5), 1.0 on columns start <=
         c < start + 5, else 0 (notebook 10's rule);
         encoder_conv = Sequential(Conv2d 5 -> 64, ReLU, Conv2d 64 -> 128, ReLU, Conv2d 128 -> 128, ReLU), all 3x3 stride 2:
         a side s becomes (s - 3) // 2 + 1 three times (128 -> 63 -> 31 -> 15);
         decoder_conv = Sequential(ConvTranspose2d 128 -> 128 stride 2, ReLU, ConvTranspose2d 128 -> 128 stride 2, ReLU,
         ConvTranspose2d 128 -> 1 stride 1): e -> 2 e + 1 -> 4 e + 3 -> 4 e + 5 (15 -> 31 -> 63 -> 65)
  loss   F.mse_loss(y_hat[:, :, :-1, :-1], target.unsqueeze(1)): the prediction is cropped, not the target; Adam(lr=1e-3)

Same attribute / state_dict names as the notebook (encoder_conv.{0,2,4}.{weight,bias}, decoder_conv.{0,2,4}.{weight,bias};
520 705 parameters).  The two nn.Sequential are parameter holders: every layer, the loss and the optimiser run on the gfx950
kernels behind include/pv_yield_hip.h (pv_conv2d_wide_s2_*, pv_convt2d_wide_s2_*, pv_convt2d_head_*, pv_mse_pred_window_f32,
pv_adam_step_f32).  The stripe plane is never stored: the first layer's kernels synthesise it from one int32 start column per
example, computed on the device as in nb10_just_conv.py, so a step can be captured as a graph.  Deliberate differences from
the notebook: it runs on the MI355X only (CPU tensors raise a RuntimeError); a target whose sides are not the output's minus
one raises a ValueError where torch would broadcast or fail inside mse_loss; a negative horizon follows the kernel rule.
"""
import torch
from torch import nn

from .._notebook_ae import NotebookAutoEncoder
from .._notebook_ae import check_target_side as _check_target_side
from ..conv3d.flow_autoencoder import FORECAST_HORIZON, HISTORICAL_SAT_IMAGES, TARGET_SAT_IMAGE  # noqa: F401

STRIDE = 2
CHANNELS = 128
N_HIST_IMAGES = 4
STRIPE_WIDTH = 128 // 24      # input img size / num timesteps
MIN_IMAGE_SIDE = 15           # 15 -> 7 -> 3 -> 1: the smallest side three 3x3 stride-2 convolutions accept


def output_side(image_side: int) -> int:
    """Side of y_hat for an input side (128 -> 65, 47 -> 25)."""
    if image_side < MIN_IMAGE_SIDE:
        raise ValueError(f"nb09 LitAutoEncoder needs images of at least {MIN_IMAGE_SIDE} x {MIN_IMAGE_SIDE} pixels (three "
                         f"3x3 stride-2 convolutions), got {image_side}")
    side = image_side
    for _ in range(3):
        side = (side - 3) // STRIDE + 1
    return 4 * side + 5       # two ConvTranspose2d at stride 2 (s -> 2 s + 1), one at stride 1 (s -> s + 2)


def target_side(image_side: int) -> int:
    """Side of the target the loss accepts: y_hat[:, :, :-1, :-1] drops the prediction's last row and column."""
    return output_side(image_side) - 1


def check_target_side(image_shape, target_shape) -> None:
    """image_shape: (H, W) of the history images; the target must be [B, target_side(H), target_side(W)]."""
    _check_target_side("nb09", target_side, image_shape, target_shape)


class LitAutoEncoder(NotebookAutoEncoder):
    name = "nb09_stripe_ae"
    nb = "nb09"
    output_side, check_target_side = staticmethod(output_side), staticmethod(check_target_side)

    def __init__(self, lr: float = 0.001):
        super().__init__()
        self.lr = float(lr)

        self.encoder_conv = nn.Sequential(
            nn.Conv2d(in_channels=N_HIST_IMAGES + 1, out_channels=CHANNELS // 2, kernel_size=3, stride=STRIDE),
            nn.ReLU(),
            nn.Conv2d(in_channels=CHANNELS // 2, out_channels=CHANNELS, kernel_size=3, stride=STRIDE),
            nn.ReLU(),
            nn.Conv2d(in_channels=CHANNELS, out_channels=CHANNELS, kernel_size=3, stride=STRIDE),
            nn.ReLU(),
        )

        self.decoder_conv = nn.Sequential(
            nn.ConvTranspose2d(in_channels=CHANNELS, out_channels=CHANNELS, kernel_size=3, stride=2),
            nn.ReLU(),
            nn.ConvTranspose2d(in_channels=CHANNELS, out_channels=CHANNELS, kernel_size=3, stride=2),
            nn.ReLU(),
            nn.ConvTranspose2d(in_channels=CHANNELS, out_channels=1, kernel_size=3, stride=1),
        )

    def forward(self, x):
        from ...conv2d_functional import nb09_stripe_ae_f32, stripe_start_from_horizon
        hist_images, horizon = self.history_and_horizon(x)
        # the stripe plane is synthesised by the first layer's kernels from one start column per example
        stripe_start = stripe_start_from_horizon(horizon, STRIPE_WIDTH)
        return nb09_stripe_ae_f32(hist_images, stripe_start, self.encoder_conv, self.decoder_conv)

    def loss(self, y_hat, y):
        from ...conv2d_functional import mse_pred_window
        # y_hat[:, :, :-1, :-1] against the target: the window of the prediction that starts at (0, 0)
        return mse_pred_window(y_hat.squeeze(1), y.to(device=y_hat.device, dtype=torch.float32), 0, 0)
