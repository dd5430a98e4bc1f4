"""Synthetic example dicts and a DataModule for notebooks/14_back_to_2d_conv_AE.ipynb and 15_int16.ipynb: the super-batches
and the example pipeline of data/nb16_datamodule.py (raw int16 counts -> flow_examples.load_super_batch(normalise=False) ->
super_batch_to_example -> collate, all on the device) with this model's target side: the centred crop of output side + 1
pixels (S = 128: 64, border 32)."""
import numpy as np

from ..models.conv2d.nb15_strided_ae import target_side
from . import flow_examples as fe
from .nb16_datamodule import Nb16DataModule, make_fake_super_batch  # noqa: F401


def make_fake_nb15_batch(super_batch, batch_size: int, image_size_pixels: int, rng: np.random.Generator):
    small = target_side(image_size_pixels)
    if (image_size_pixels - small) % 2:
        raise ValueError(f"image_size_pixels={image_size_pixels}: the centred target crop of {small} pixels needs an even "
                         f"border")
    examples = [fe.super_batch_to_example(super_batch, rng, n_pixels_per_side_large=image_size_pixels,
                                          n_pixels_per_side_small=small) for _ in range(batch_size)]
    return fe.collate(examples)


class Nb15DataModule(Nb16DataModule):
    """Nb16DataModule with the stride-2 model's target crop."""

    make_batch = staticmethod(make_fake_nb15_batch)
