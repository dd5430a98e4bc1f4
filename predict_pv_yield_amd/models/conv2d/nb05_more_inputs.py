"""LitAutoEncoder whose inputs are the optical-flow prediction, the t0 image and the flow field itself -- host-side mirror of
notebooks/05_more_image_inputs.ipynb (the cell that defines LitAutoEncoder with STRIDE = 1, GROUPS = 1, CHANNELS = 32, raw
lines 1348-1408 of the .ipynb file; the three nn.Conv2d at 1357-1361, the three nn.ConvTranspose2d at 1366-1370).

  input  x['input_images']      [B, 1, H, W]     float32, the flow-advected prediction, normalised (H = W = 64 in the notebook)
         x['T0_IMAGES']         [B, 1, H, W]     float32, the image the prediction was advected from, normalised
         x['optical_flow']      [B, 1, 2, H, W]  float32, planar x then y displacement in pixels, not normalised; [B, 2, H, W]
                                                 is accepted too
         x['forecast_horizon']  [B]              float32, normalised by the loader ((minutes - 62.5) / 34.61)
         x['target_images']     [B, 1, H, W]     float32, normalised
  graph  x_cat = cat(input_images, T0_IMAGES, optical_flow without its singleton axis): [B, 4, H, W];
         encoder = Sequential(Conv2d 4 -> 32, ReLU, Conv2d 32 -> 32, ReLU, Conv2d 32 -> 32, ReLU), 3x3, no padding: a side s
         becomes s - 2 three times (64 -> 58); the horizon joins as a 33rd, constant channel;
         decoder = Sequential(ConvTranspose2d 33 -> 32, ReLU, ConvTranspose2d 32 -> 32, ReLU, ConvTranspose2d 32 -> 1), 3x3,
         stride 1: s -> s + 2 three times (58 -> 64), so y_hat has the input's sides
  loss   F.mse_loss(y_hat, target_images), both [B, 1, H, W]; Adam(lr=1e-3)

Same attribute / state_dict names as the notebook (encoder.{0,2,4}.{weight,bias}, decoder.{0,2,4}.{weight,bias}; 38 753
parameters).  The two nn.Sequential are parameter holders: every layer, the loss and the optimiser run on the gfx950 kernels
behind include/pv_yield_hip.h (pv_conv2d_ae_inputs_*, pv_conv2d_ae_*, pv_convt2d_ae_horizon_*, pv_convt2d_ae_*,
pv_convt2d_head_*, pv_mse_pred_window_f32, pv_adam_step_f32).  Neither x_cat nor the 33-channel decoder input is ever stored:
the first layer's kernels read the three tensors in place, and the first decoder layer's kernels read the horizon of each
example from device memory, so a step can be captured as a graph.  Deliberate differences from the notebook: it runs on the
MI355X only (CPU tensors raise a RuntimeError); the batch axis survives B = 1 (the notebook's optical_flow.squeeze() drops it
together with the singleton axis, after which torch.cat fails); and mis-shaped inputs or targets raise a ValueError where torch
would broadcast or fail inside cat / mse_loss.
"""
import torch
from torch import nn

from .._notebook_ae import NotebookAutoEncoder

STRIDE = 1
GROUPS = 1
CHANNELS = 32
MIN_IMAGE_SIDE = 7            # 7 -> 5 -> 3 -> 1: the smallest side three 3x3 convolutions accept
MAX_IMAGE_SIDE = 128          # the kernels' widest plane

# the batch keys, as the notebook spells them
INPUT_IMAGES = 'input_images'
T0_IMAGES = 'T0_IMAGES'
OPTICAL_FLOW = 'optical_flow'
FORECAST_HORIZON = 'forecast_horizon'
TARGET_IMAGES = 'target_images'


def output_side(image_side: int) -> int:
    """Side of y_hat for an input side: the same (64 -> 58 -> 64)."""
    if not MIN_IMAGE_SIDE <= image_side <= MAX_IMAGE_SIDE:
        raise ValueError(f"nb05 LitAutoEncoder needs images of {MIN_IMAGE_SIDE} to {MAX_IMAGE_SIDE} pixels a side (three 3x3 "
                         f"convolutions; planes up to {MAX_IMAGE_SIDE} wide), got {image_side}")
    return image_side         # three 3x3 convolutions take 6 off, three stride-1 transposed ones put them back


def check_target_side(image_shape, target_shape) -> None:
    """image_shape: (H, W) of the input images; the target must be [B, 1, H, W], the shape of y_hat."""
    want = tuple(output_side(int(side)) for side in image_shape)
    if len(target_shape) != 4 or tuple(target_shape[1:]) != (1,) + want:
        raise ValueError(f"nb05 LitAutoEncoder: {TARGET_IMAGES} must be [B, 1, {want[0]}, {want[1]}] for {image_shape[0]} x "
                         f"{image_shape[1]}-pixel inputs, got {tuple(target_shape)}")


class LitAutoEncoder(NotebookAutoEncoder):
    name = "nb05_more_inputs"
    nb = "nb05"
    image_key, target_key = INPUT_IMAGES, TARGET_IMAGES
    output_side, check_target_side = staticmethod(output_side), staticmethod(check_target_side)

    def __init__(self, lr: float = 0.001):
        super().__init__()
        self.lr = float(lr)

        self.encoder = nn.Sequential(
            nn.Conv2d(in_channels=4, out_channels=CHANNELS, kernel_size=3, stride=STRIDE, groups=GROUPS),
            nn.ReLU(),
            nn.Conv2d(in_channels=CHANNELS, out_channels=CHANNELS, kernel_size=3, stride=STRIDE, groups=GROUPS),
            nn.ReLU(),
            nn.Conv2d(in_channels=CHANNELS, out_channels=CHANNELS, kernel_size=3, stride=STRIDE, groups=GROUPS),
            nn.ReLU(),
        )

        self.decoder = nn.Sequential(
            nn.ConvTranspose2d(in_channels=CHANNELS + 1, out_channels=CHANNELS, kernel_size=3, stride=STRIDE),
            nn.ReLU(),
            nn.ConvTranspose2d(in_channels=CHANNELS, out_channels=CHANNELS, kernel_size=3, stride=STRIDE),
            nn.ReLU(),
            nn.ConvTranspose2d(in_channels=CHANNELS, out_channels=1, kernel_size=3, stride=STRIDE),
        )

    def forward(self, x):
        from ...conv2d_functional import nb05_more_inputs_f32
        # x_cat and the horizon channel are synthesised by the first encoder / decoder layers' kernels
        inputs = self.flow_inputs_and_horizon(x, INPUT_IMAGES, T0_IMAGES, OPTICAL_FLOW, FORECAST_HORIZON)
        return nb05_more_inputs_f32(*inputs, self.encoder, self.decoder)

    def loss(self, y_hat, y):
        from ...conv2d_functional import mse_pred_window
        # prediction and target have the same sides: the window is all of y_hat
        return mse_pred_window(y_hat.squeeze(1), y.to(device=y_hat.device, dtype=torch.float32).squeeze(1), 0, 0)
