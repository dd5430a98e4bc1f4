"""Super-batch -> training-example pipeline of notebooks/05_more_image_inputs.ipynb on the device, and a seeded DataModule of
synthetic batches (the notebook's own SatelliteLoader streams a zarr store from a bucket, outside the hot path).

  flow_examples.load_super_batch   SatelliteLoader.load_super_batch: Farneback fields on the raw counts, normalised images, all
                                   (n - 1) n / 2 flow predictions (NaN border) and their (t0, target) index
  pick_example_indices             host half of super_batch_to_example (pure NumPy): which prediction, which t0 / target image,
                                   which flow field, and the normalised horizon
  sample_squares                   device half: one random square cut from the prediction, the target, the flow field and the t0
                                   image alike; a square that holds a NaN is drawn again
  super_batch_to_example           the two together -> the notebook's five keys

An example keeps the notebook's keys and shapes: 'input_images', 'target_images' and 'T0_IMAGES' [1, s, s], 'optical_flow' [1, 2,
s, s] (planar, x displacement then y), 'forecast_horizon' a float32 scalar; flow_examples.collate stacks B of them.  The images
never leave the MI355X: the crops are views of device tensors, and only the index choices (numpy Generator, drawn in the
notebook's order) run on the host.

Reproduced from the notebook on purpose: the flow field is the one at the *target* index, clipped to the last field
(super_batch_to_example: target_idx.clip(max=n_optical_flows - 1)), not the field the prediction was advected with; and the
horizon is in minutes, normalised in float32 as (m - 62.5) / 34.61 (subtract, then divide).  One deliberate difference: after
1000 squares with NaNs the notebook silently keeps the last one; here that raises ImageHasNansError."""
from typing import Dict, Optional

import numpy as np
import torch

from ..models.conv2d.nb05_more_inputs import FORECAST_HORIZON, INPUT_IMAGES, OPTICAL_FLOW, T0_IMAGES, TARGET_IMAGES
from . import flow_examples as fe
from .flow_examples import ImageHasNansError
from .nb16_datamodule import Nb16DataModule
from .synthetic import advected_counts

MINUTES_PER_TIMESTEP = 5
HORIZON_MEAN_MINUTES = np.float32(62.5)
HORIZON_STD_MINUTES = np.float32(34.61)
NUM_CROP_RETRIES = 1000


def normalise_forecast_horizon(minutes) -> np.float32:
    """forecast_horizon.astype(np.float32); forecast_horizon -= 62.5; forecast_horizon /= 34.61, every step in float32."""
    horizon = np.float32(minutes)
    horizon = np.float32(horizon - HORIZON_MEAN_MINUTES)
    return np.float32(horizon / HORIZON_STD_MINUTES)


def pick_example_indices(prediction_index: np.ndarray, n_flows: int, row: int):
    """Host half of super_batch_to_example for prediction `row` of prediction_index [P, 2] = (t0 index, target index): (t0
    index, target index, flow field index, normalised horizon).  The flow field is the one at the target index, clipped to the
    last field, as in the notebook."""
    t0_idx, target_idx = (int(v) for v in prediction_index[row])
    flow_idx = min(target_idx, n_flows - 1)
    return t0_idx, target_idx, flow_idx, normalise_forecast_horizon((target_idx - t0_idx) * MINUTES_PER_TIMESTEP)


def draw_example_indices(rng: np.random.Generator, prediction_index: np.ndarray, n_flows: int):
    """InMemDataset.__iter__'s draw, input_idx = rng.integers(low=0, high=n_input_images): uniform over all P predictions.
    Returns (row, *pick_example_indices(row))."""
    row = int(rng.integers(low=0, high=len(prediction_index)))
    return (row, *pick_example_indices(prediction_index, n_flows, row))


def sample_squares(example: Dict[str, torch.Tensor], rng: np.random.Generator, n_pixels_per_side: int = 64,
                   max_retries: int = NUM_CROP_RETRIES) -> Dict[str, torch.Tensor]:
    """Device half.  example: INPUT_IMAGES, TARGET_IMAGES and T0_IMAGES [1, H, W], OPTICAL_FLOW [1, H, W, 2] (the field as
    load_super_batch keeps it).  One (top, left) is shared by all four crops, top drawn before left; the field's crop is
    returned planar, [1, 2, s, s]."""
    height, width = example[INPUT_IMAGES].shape[-2:]
    max_x, max_y = width - n_pixels_per_side, height - n_pixels_per_side
    for _ in range(max_retries):
        top = int(rng.integers(low=0, high=max_y))
        left = int(rng.integers(low=0, high=max_x))
        rows, cols = slice(top, top + n_pixels_per_side), slice(left, left + n_pixels_per_side)
        crops = {INPUT_IMAGES: example[INPUT_IMAGES][..., rows, cols],     # first: the most likely to have NaNs
                 TARGET_IMAGES: example[TARGET_IMAGES][..., rows, cols],
                 OPTICAL_FLOW: example[OPTICAL_FLOW][..., rows, cols, :].movedim(-1, -3),
                 T0_IMAGES: example[T0_IMAGES][..., rows, cols]}
        if not any(bool(torch.isnan(c).any()) for c in crops.values()):
            return {**example, **crops}
    raise ImageHasNansError(f"Cropped images still have NaNs, even after {max_retries} retries!")


def super_batch_to_example(super_batch: Dict[str, torch.Tensor], rng: Optional[np.random.Generator] = None,
                           n_pixels_per_side: int = 64, max_retries: int = NUM_CROP_RETRIES) -> Dict[str, torch.Tensor]:
    """One example from flow_examples.load_super_batch's dict (images normalised there)."""
    rng = rng if rng is not None else np.random.default_rng()
    sat, fields = super_batch[fe.SAT_IMAGES], super_batch[fe.OPTICAL_FLOW_FIELDS]
    index = super_batch[fe.PREDICTION_INDEX]
    index = index.cpu().numpy() if isinstance(index, torch.Tensor) else np.asarray(index)
    row, t0_idx, target_idx, flow_idx, horizon = draw_example_indices(rng, index, len(fields))
    example = {INPUT_IMAGES: super_batch[fe.OPTICAL_FLOW_PREDICTIONS][row][None],
               TARGET_IMAGES: sat[target_idx][None],
               OPTICAL_FLOW: fields[flow_idx][None],
               FORECAST_HORIZON: torch.tensor(horizon, device=sat.device),
               T0_IMAGES: sat[t0_idx][None]}
    return sample_squares(example, rng, n_pixels_per_side, max_retries)


def make_fake_super_batch(device, n_timesteps: int = 16, frame_size_pixels: int = 176, seed: int = 1234):
    """One synthetic super-batch: [T, H, W] advected texture normalised in the loader, its flow fields (computed on the raw
    counts) and all flow predictions."""
    raw, _ = advected_counts(batch=1, t=n_timesteps, channels=1, h=frame_size_pixels, w=frame_size_pixels, seed=seed)
    counts = torch.from_numpy(np.ascontiguousarray(raw[0, :, 0])).to(device)
    return fe.load_super_batch(counts, normalise=True)


def make_fake_nb05_batch(super_batch, batch_size: int, image_size_pixels: int, rng: np.random.Generator):
    return fe.collate([super_batch_to_example(super_batch, rng, image_size_pixels) for _ in range(batch_size)])


class Nb05DataModule(Nb16DataModule):
    """Nb16DataModule's seeded scheme (n_train_data / n_val_data batches drawn from n_super_batches synthetic super-batches,
    built once on the device at setup()) with normalised super-batches and notebook 05's examples."""

    make_batch = staticmethod(make_fake_nb05_batch)
    make_super_batch = staticmethod(make_fake_super_batch)

    def __init__(self, batch_size: int = 64, image_size_pixels: int = 64, **kwargs):
        super().__init__(batch_size=batch_size, image_size_pixels=image_size_pixels, **kwargs)

    def setup(self, stage=None):
        if self._train is not None:
            return
        supers = [self.make_super_batch(self.device, self.n_timesteps, self.frame_size_pixels, self.seed + i)
                  for i in range(self.n_super_batches)]
        rng = np.random.default_rng(self.seed)

        def batches(n):
            return [self.make_batch(supers[int(rng.integers(len(supers)))], self.batch_size, self.image_size_pixels, rng)
                    for _ in range(n)]

        self._train, self._val = batches(self.n_train_data), batches(self.n_val_data)
