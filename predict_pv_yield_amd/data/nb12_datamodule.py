"""Synthetic example dicts and a DataModule for notebooks/12_just_3d_conv.ipynb.  The super-batches and the order of draws
are those of data/nb10_datamodule.py (make_fake_super_batch, draw_example: the notebook's super_batch_to_example /
sample_squares cells are the same in both notebooks); what differs is FORECAST_HORIZON, which this notebook normalises in the
loader (normalise_forecast_horizon, 12_just_3d_conv.ipynb:757-768): float32 (h - mean) / std of arange(1, 25).  The batch
keeps the notebook's three keys: HISTORICAL_SAT_IMAGES [B, 4, S, S] f32, FORECAST_HORIZON [B] f32, TARGET_SAT_IMAGE [B, s, s]
f32 with s = (S - 1) // 2 + 1."""
import numpy as np
import torch

from ..models.conv3d.nb12_just_3d_conv import (FORECAST_HORIZON, HISTORICAL_SAT_IMAGES, N_HIST_IMAGES, TARGET_SAT_IMAGE,
                                               output_side)
from .nb10_datamodule import Nb10DataModule, draw_example, make_fake_super_batch  # noqa: F401

FCST_HORIZON_SEQ = np.arange(1, 25, dtype=np.float32)
FCST_HORIZON_MEAN = FCST_HORIZON_SEQ.mean()
FCST_HORIZON_STD = FCST_HORIZON_SEQ.std()


def normalise_forecast_horizon(forecast_horizon: int) -> np.float32:
    """Timesteps 1..24 (5 minutes each) to the notebook's float32 network input."""
    forecast_horizon = np.float32(forecast_horizon)
    forecast_horizon -= FCST_HORIZON_MEAN
    forecast_horizon /= FCST_HORIZON_STD
    return forecast_horizon


def super_batch_to_example(frames: np.ndarray, rng: np.random.Generator, side_large: int = 128, side_small: int = 64):
    n_frames, height, width = frames.shape
    hist_start, horizon, top, left = draw_example(n_frames, height, width, rng, side_large, N_HIST_IMAGES)
    hist_end = hist_start + N_HIST_IMAGES
    border = (side_large - side_small) // 2
    target = frames[hist_end - 1 + horizon, top + border:top + side_large - border, left + border:left + side_large - border]
    return {TARGET_SAT_IMAGE: target, FORECAST_HORIZON: normalise_forecast_horizon(horizon),
            HISTORICAL_SAT_IMAGES: frames[hist_start:hist_end, top:top + side_large, left:left + side_large]}


def make_fake_nb12_batch(frames: np.ndarray, batch_size: int, image_size_pixels: int, rng: np.random.Generator, device):
    small = output_side(image_size_pixels)
    if (image_size_pixels - small) % 2:
        raise ValueError(f"image_size_pixels={image_size_pixels}: the centred target crop of {small} pixels needs an even "
                         f"border")
    examples = [super_batch_to_example(frames, rng, image_size_pixels, small) for _ in range(batch_size)]
    return {HISTORICAL_SAT_IMAGES: torch.from_numpy(np.stack([e[HISTORICAL_SAT_IMAGES] for e in examples])).to(device),
            FORECAST_HORIZON: torch.from_numpy(np.array([e[FORECAST_HORIZON] for e in examples], dtype=np.float32)).to(device),
            TARGET_SAT_IMAGE: torch.from_numpy(np.stack([e[TARGET_SAT_IMAGE] for e in examples])).to(device)}


class Nb12DataModule(Nb10DataModule):
    """Nb10DataModule's seeded batches (same super-batches, same draws) with the horizon normalised as notebook 12 does."""

    def setup(self, stage=None):
        if self._train is not None:
            return
        supers = [make_fake_super_batch(self.n_timesteps, self.frame_size_pixels, self.seed + i)
                  for i in range(self.n_super_batches)]
        rng = np.random.default_rng(self.seed)

        def batches(n):
            return [make_fake_nb12_batch(supers[int(rng.integers(len(supers)))], self.batch_size, self.image_size_pixels, rng,
                                         self.device) for _ in range(n)]

        self._train, self._val = batches(self.n_train_data), batches(self.n_val_data)
