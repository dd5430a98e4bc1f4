"""Synthetic example dicts and a DataModule for notebooks/10_just_conv.ipynb (the notebook's own SatelliteLoader streams a
zarr store from a bucket, outside the hot path).  A super-batch is [T, H, W] of advected dense texture (data/synthetic.py),
normalised in the loader as the notebook's normalise_images does; an example follows the notebook's super_batch_to_example /
sample_squares cells draw for draw: the first of 4 consecutive history frames, the horizon rng.integers(1, min(n - hist_end,
24)), the target frame t0 + horizon, then the top and left of the 128-pixel history crop, whose centred 64-pixel crop is the
target.  (The notebook retries a crop that holds NaNs; the synthetic frames hold none, so the first draw stands.)  The batch
keeps the notebook's three keys: HISTORICAL_SAT_IMAGES [B, 4, S, S] f32, FORECAST_HORIZON [B] int64, TARGET_SAT_IMAGE [B, s,
s] f32."""
import numpy as np
import torch

from ..lightning import LightningDataModule
from ..models.conv2d.nb10_just_conv import (FORECAST_HORIZON, HISTORICAL_SAT_IMAGES, N_HIST_IMAGES, TARGET_SAT_IMAGE,
                                            output_side)
from .synthetic import advected_counts

SAT_IMAGE_MEAN = 93.23458
SAT_IMAGE_STD = 115.34247
MAX_HORIZON = 24


def make_fake_super_batch(n_timesteps: int = 49, frame_size_pixels: int = 176, seed: int = 1234) -> np.ndarray:
    """One synthetic super-batch [T, H, W] float32, normalised (10_just_conv.ipynb: normalise_images)."""
    raw, _ = advected_counts(batch=1, t=n_timesteps, channels=1, h=frame_size_pixels, w=frame_size_pixels, seed=seed)
    frames = np.ascontiguousarray(raw[0, :, 0]).astype(np.float32)
    frames -= np.float32(SAT_IMAGE_MEAN)
    frames /= np.float32(SAT_IMAGE_STD)
    return frames


def draw_example(n_frames: int, height: int, width: int, rng: np.random.Generator, side_large: int = 128,
                 history_length: int = N_HIST_IMAGES):
    """(hist_start, horizon, top, left) in the notebook's order of draws."""
    hist_start = int(rng.integers(low=0, high=n_frames - history_length - 1))
    hist_end = hist_start + history_length
    horizon = int(rng.integers(low=1, high=min(n_frames - hist_end, MAX_HORIZON)))
    top = int(rng.integers(low=0, high=height - side_large))
    left = int(rng.integers(low=0, high=width - side_large))
    return hist_start, horizon, top, left


def super_batch_to_example(frames: np.ndarray, rng: np.random.Generator, side_large: int = 128, side_small: int = 64,
                           horizon_form=int):
    """One example: the history crop, its centred target crop and horizon_form(timesteps ahead)."""
    n_frames, height, width = frames.shape
    hist_start, horizon, top, left = draw_example(n_frames, height, width, rng, side_large)
    hist_end = hist_start + N_HIST_IMAGES
    border = (side_large - side_small) // 2
    target = frames[hist_end - 1 + horizon, top + border:top + side_large - border, left + border:left + side_large - border]
    return {TARGET_SAT_IMAGE: target, FORECAST_HORIZON: horizon_form(horizon),
            HISTORICAL_SAT_IMAGES: frames[hist_start:hist_end, top:top + side_large, left:left + side_large]}


def make_fake_batch(frames: np.ndarray, batch_size: int, image_size_pixels: int, rng: np.random.Generator, device,
                    side_rule=output_side, horizon_form=int):
    """batch_size examples whose centred target crop has side_rule(image_size_pixels) pixels a side; the horizon is int64 where
    horizon_form leaves it an int, else float32."""
    small = side_rule(image_size_pixels)
    if (image_size_pixels - small) % 2:
        raise ValueError(f"image_size_pixels={image_size_pixels}: the centred target crop of {small} pixels needs an even "
                         f"border")
    examples = [super_batch_to_example(frames, rng, image_size_pixels, small, horizon_form) for _ in range(batch_size)]
    horizon = np.array([e[FORECAST_HORIZON] for e in examples])
    return {HISTORICAL_SAT_IMAGES: torch.from_numpy(np.stack([e[HISTORICAL_SAT_IMAGES] for e in examples])).to(device),
            FORECAST_HORIZON: torch.from_numpy(horizon).to(device),
            TARGET_SAT_IMAGE: torch.from_numpy(np.stack([e[TARGET_SAT_IMAGE] for e in examples])).to(device)}


make_fake_nb10_batch = make_fake_batch


class Nb10DataModule(LightningDataModule):
    """n_train_data / n_val_data seeded batches drawn from n_super_batches synthetic super-batches, built once at setup().
    make_batch: the model's batch builder (a subclass sets its own target side and horizon form)."""

    make_batch = staticmethod(make_fake_nb10_batch)

    def __init__(self, batch_size: int = 64, image_size_pixels: int = 128, n_train_data: int = 8, n_val_data: int = 2,
                 n_super_batches: int = 2, n_timesteps: int = 49, frame_size_pixels: int = 176, seed: int = 1234,
                 device: str = "cuda"):
        super().__init__()
        self.batch_size, self.image_size_pixels = batch_size, image_size_pixels
        self.n_train_data, self.n_val_data, self.n_super_batches = n_train_data, n_val_data, n_super_batches
        self.n_timesteps, self.frame_size_pixels, self.seed, self.device = n_timesteps, frame_size_pixels, seed, device
        self._train = self._val = None

    def setup(self, stage=None):
        if self._train is not None:
            return
        supers = [make_fake_super_batch(self.n_timesteps, self.frame_size_pixels, self.seed + i)
                  for i in range(self.n_super_batches)]
        rng = np.random.default_rng(self.seed)

        def batches(n):
            return [self.make_batch(supers[int(rng.integers(len(supers)))], self.batch_size, self.image_size_pixels, rng,
                                    self.device) for _ in range(n)]

        self._train, self._val = batches(self.n_train_data), batches(self.n_val_data)

    @staticmethod
    def _loader(items):
        return torch.utils.data.DataLoader(items, batch_size=None, num_workers=0)

    def train_dataloader(self):
        self.setup()
        return self._loader(self._train)

    def val_dataloader(self):
        self.setup()
        return self._loader(self._val)

    def test_dataloader(self):
        return self.val_dataloader()
