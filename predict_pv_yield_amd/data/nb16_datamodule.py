"""Synthetic example dicts and a DataModule for notebooks/16_maxpool.ipynb (the notebook's own SatelliteLoader streams a
zarr store from a bucket, outside the hot path): advected dense textures (data/synthetic.py, as config 3 makes them) as raw
int16 counts -> flow_examples.load_super_batch(normalise=False) -> super_batch_to_example -> collate, all on the device.
The batches keep the notebook's four keys with HISTORICAL_SAT_IMAGES / TARGET_SAT_IMAGE as int16 counts and
OPTICAL_FLOW_PREDICTIONS as float32 counts; the model normalises by itself."""
import numpy as np
import torch

from ..lightning import LightningDataModule
from ..models.conv2d.nb16_maxpool import target_side
from . import flow_examples as fe
from .synthetic import advected_counts


def make_fake_super_batch(device, n_timesteps: int = 16, frame_size_pixels: int = 176, seed: int = 1234):
    """One synthetic super-batch in raw counts: [T, H, W] advected texture, its flow fields and all flow predictions."""
    raw, _ = advected_counts(batch=1, t=n_timesteps, channels=1, h=frame_size_pixels, w=frame_size_pixels, seed=seed)
    counts = torch.from_numpy(np.ascontiguousarray(raw[0, :, 0])).to(device)
    return fe.load_super_batch(counts, normalise=False)


def make_fake_nb16_batch(super_batch, batch_size: int, image_size_pixels: int, rng: np.random.Generator):
    small = target_side(image_size_pixels)
    if (image_size_pixels - small) % 2:
        raise ValueError(f"image_size_pixels={image_size_pixels}: the centred target crop of {small} pixels needs an even "
                         f"border")
    examples = [fe.super_batch_to_example(super_batch, rng, n_pixels_per_side_large=image_size_pixels,
                                          n_pixels_per_side_small=small) for _ in range(batch_size)]
    return fe.collate(examples)


class Nb16DataModule(LightningDataModule):
    """n_train_data / n_val_data seeded batches drawn from n_super_batches synthetic super-batches, built once on the device
    at setup().  make_batch: the model's batch builder (a subclass sets its own target crop)."""

    make_batch = staticmethod(make_fake_nb16_batch)

    def __init__(self, batch_size: int = 64, image_size_pixels: int = 128, n_train_data: int = 8, n_val_data: int = 2,
                 n_super_batches: int = 2, n_timesteps: int = 16, frame_size_pixels: int = 176, seed: int = 1234,
                 device: str = "cuda"):
        super().__init__()
        self.batch_size, self.image_size_pixels = batch_size, image_size_pixels
        self.n_train_data, self.n_val_data, self.n_super_batches = n_train_data, n_val_data, n_super_batches
        self.n_timesteps, self.frame_size_pixels, self.seed, self.device = n_timesteps, frame_size_pixels, seed, device
        self._train = self._val = None

    def setup(self, stage=None):
        if self._train is not None:
            return
        supers = [make_fake_super_batch(self.device, self.n_timesteps, self.frame_size_pixels, self.seed + i)
                  for i in range(self.n_super_batches)]
        rng = np.random.default_rng(self.seed)

        def batches(n):
            return [self.make_batch(supers[int(rng.integers(len(supers)))], self.batch_size, self.image_size_pixels, rng)
                    for _ in range(n)]

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
