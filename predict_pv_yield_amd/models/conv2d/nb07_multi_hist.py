"""LitAutoEncoder of the weight-shared per-frame encoder / ConvTranspose2d decoder -- host-side mirror of
notebooks/07_multiple_historical_images.ipynb (the cell that defines LitAutoEncoder with STRIDE = 2, CHANNELS = 32,
N_HIST_IMAGES = 4, raw lines 1356-1415 of the .ipynb file; the three nn.Conv2d at 1365-1369, the three nn.ConvTranspose2d at
1374-1378, forward at 1381-1396).

  input  x[HISTORICAL_SAT_IMAGES]  [B, 4, H, W]   float32, normalised by the loader (H = W = 128 in the notebook)
         x[FORECAST_HORIZON]       [B]            float32, normalised by the loader
         x[TARGET_SAT_IMAGE]       [B, h_t, w_t]  float32, normalised; (h_t, w_t) == the output's sides - 1 (H = 128: 64)
  graph  every history frame f, with the horizon as a second, constant channel, goes through the same
         encoder_conv = Sequential(Conv2d 2 -> 32, ReLU, Conv2d 32 -> 32, ReLU, Conv2d 32 -> 32, ReLU), all 3x3, stride 2, no
         padding: a side s becomes (s - 3) // 2 + 1 three times (128 -> 63 -> 31 -> 15); the four outputs are concatenated
         along the channels;
         decoder_conv = Sequential(ConvTranspose2d 128 -> 32 stride 2, ReLU, ConvTranspose2d 32 -> 32 stride 2, ReLU,
         ConvTranspose2d 32 -> 1 stride 1): e -> 2 e + 1 -> 4 e + 3 -> 4 e + 5 (15 -> 31 -> 63 -> 65)
  loss   F.mse_loss(y_hat[:, :, :-1, :-1], target.unsqueeze(1)): the prediction is cropped, not the target; Adam(lr=1e-3)

Same attribute / state_dict names as the notebook (encoder_conv.{0,2,4}.{weight,bias}, decoder_conv.{0,2,4}.{weight,bias};
65 537 parameters).  The two nn.Sequential are parameter holders: every layer, the loss and the optimiser run on the gfx950
kernels behind include/pv_yield_hip.h (pv_conv2d_s2_frame_horizon_*, pv_conv2d_s2_*, pv_convt2d_s2_frames_*, pv_convt2d_s2_*,
pv_convt2d_head_*, pv_mse_pred_window_f32, pv_adam_step_f32).  The encoder runs once over 4 B images (image 4 b + f) instead
of four times over B, so each of its parameters receives the sum of the four calls' gradients from one weight-gradient pass;
neither the two-channel encoder inputs nor the concatenated encoder output is ever written (the first is synthesised by the
first layer's kernels, which read the horizon of each example from device memory so that a step can be captured as a graph;
the second is a view).  Deliberate differences from the notebook: it runs on the MI355X only (CPU tensors raise a
RuntimeError), and a target whose sides are not the output's minus one raises a ValueError where torch would broadcast or
fail inside mse_loss.
"""
import torch
from torch import nn

from .._notebook_ae import NotebookAutoEncoder
from .._notebook_ae import check_target_side as _check_target_side
from ..conv3d.flow_autoencoder import FORECAST_HORIZON, HISTORICAL_SAT_IMAGES, TARGET_SAT_IMAGE  # noqa: F401

STRIDE = 2
CHANNELS = 32
N_HIST_IMAGES = 4
MIN_IMAGE_SIDE = 15           # 15 -> 7 -> 3 -> 1: the smallest side three 3x3 stride-2 convolutions accept
MAX_IMAGE_SIDE = 128          # the kernels' widest plane


def output_side(image_side: int) -> int:
    """Side of y_hat for an input side (128 -> 65, 31 -> 17, 15 -> 9)."""
    if not MIN_IMAGE_SIDE <= image_side <= MAX_IMAGE_SIDE:
        raise ValueError(f"nb07 LitAutoEncoder needs images of {MIN_IMAGE_SIDE} to {MAX_IMAGE_SIDE} pixels a side (three 3x3 "
                         f"stride-2 convolutions; planes up to {MAX_IMAGE_SIDE} wide), got {image_side}")
    side = image_side
    for _ in range(3):
        side = (side - 3) // 2 + 1
    return 4 * side + 5       # two ConvTranspose2d at stride 2 (s -> 2 s + 1), one at stride 1 (s -> s + 2)


def target_side(image_side: int) -> int:
    """Side of the target the loss accepts: y_hat[:, :, :-1, :-1] drops the prediction's last row and column."""
    return output_side(image_side) - 1


def check_target_side(image_shape, target_shape) -> None:
    """image_shape: (H, W) of the history images; the target must be [B, target_side(H), target_side(W)]."""
    _check_target_side("nb07", target_side, image_shape, target_shape)


class LitAutoEncoder(NotebookAutoEncoder):
    name = "nb07_multi_hist"
    nb = "nb07"
    output_side, check_target_side = staticmethod(output_side), staticmethod(check_target_side)

    def __init__(self, lr: float = 0.001):
        super().__init__()
        self.lr = float(lr)

        self.encoder_conv = nn.Sequential(
            nn.Conv2d(in_channels=2, out_channels=CHANNELS, kernel_size=3, stride=STRIDE),
            nn.ReLU(),
            nn.Conv2d(in_channels=CHANNELS, out_channels=CHANNELS, kernel_size=3, stride=STRIDE),
            nn.ReLU(),
            nn.Conv2d(in_channels=CHANNELS, out_channels=CHANNELS, kernel_size=3, stride=STRIDE),
            nn.ReLU(),
        )

        self.decoder_conv = nn.Sequential(
            nn.ConvTranspose2d(in_channels=CHANNELS * N_HIST_IMAGES, out_channels=CHANNELS, kernel_size=3, stride=2),
            nn.ReLU(),
            nn.ConvTranspose2d(in_channels=CHANNELS, out_channels=CHANNELS, kernel_size=3, stride=2),
            nn.ReLU(),
            nn.ConvTranspose2d(in_channels=CHANNELS, out_channels=1, kernel_size=3, stride=1),
        )

    def forward(self, x):
        from ...conv2d_functional import nb07_multi_hist_f32
        # the horizon channel of every frame is synthesised by the first layer's kernels from one value per example
        return nb07_multi_hist_f32(*self.history_and_horizon(x, torch.float32), self.encoder_conv, self.decoder_conv)

    def loss(self, y_hat, y):
        from ...conv2d_functional import mse_pred_window
        # y_hat[:, :, :-1, :-1] against the target: the window of the prediction that starts at (0, 0)
        return mse_pred_window(y_hat.squeeze(1), y.to(device=y_hat.device, dtype=torch.float32), 0, 0)
