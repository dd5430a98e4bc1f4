"""Synthetic example dicts and a DataModule for notebooks/08_multiple_historical_images_as_separate_channels.ipynb.  The
super-batches, the order of draws and the normalised FORECAST_HORIZON are those of data/nb12_datamodule.py (the notebooks'
super_batch_to_example / sample_squares / normalise_forecast_horizon cells are the same); what differs is the side of the
centred target crop, which follows this model's rule: three stride-2 convolutions, three transposed ones, and the loss drops
the prediction's last row and column (128 -> 64, as in notebook 12, but 42 -> 20 where notebook 12's rule gives 21).  The
batch keeps the notebook's three keys: HISTORICAL_SAT_IMAGES [B, 4, S, S] f32, FORECAST_HORIZON [B] f32, TARGET_SAT_IMAGE [B,
s, s] f32 with s = target_side(S)."""
import numpy as np
import torch

from ..models.conv3d.nb08_hist_depth import FORECAST_HORIZON, HISTORICAL_SAT_IMAGES, TARGET_SAT_IMAGE, target_side
from .nb12_datamodule import Nb12DataModule, make_fake_super_batch, super_batch_to_example


def make_fake_nb08_batch(frames: np.ndarray, batch_size: int, image_size_pixels: int, rng: np.random.Generator, device):
    small = target_side(image_size_pixels)
    if (image_size_pixels - small) % 2:
        raise ValueError(f"image_size_pixels={image_size_pixels}: the centred target crop of {small} pixels needs an even "
                         f"border")
    examples = [super_batch_to_example(frames, rng, image_size_pixels, small) for _ in range(batch_size)]
    return {HISTORICAL_SAT_IMAGES: torch.from_numpy(np.stack([e[HISTORICAL_SAT_IMAGES] for e in examples])).to(device),
            FORECAST_HORIZON: torch.from_numpy(np.array([e[FORECAST_HORIZON] for e in examples], dtype=np.float32)).to(device),
            TARGET_SAT_IMAGE: torch.from_numpy(np.stack([e[TARGET_SAT_IMAGE] for e in examples])).to(device)}


class Nb08DataModule(Nb12DataModule):
    """Nb12DataModule's seeded batches (same super-batches, same draws, same horizon) with notebook 08's target side."""

    def setup(self, stage=None):
        if self._train is not None:
            return
        supers = [make_fake_super_batch(self.n_timesteps, self.frame_size_pixels, self.seed + i)
                  for i in range(self.n_super_batches)]
        rng = np.random.default_rng(self.seed)

        def batches(n):
            return [make_fake_nb08_batch(supers[int(rng.integers(len(supers)))], self.batch_size, self.image_size_pixels, rng,
                                         self.device) for _ in range(n)]

        self._train, self._val = batches(self.n_train_data), batches(self.n_val_data)
