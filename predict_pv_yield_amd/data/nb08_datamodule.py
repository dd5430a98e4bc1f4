"""Synthetic example dicts and a DataModule for notebooks/08_multiple_historical_images_as_separate_channels.ipynb.  The
super-batches, the order of draws and the normalised FORECAST_HORIZON are those of data/nb12_datamodule.py (the notebooks'
super_batch_to_example / sample_squares / normalise_forecast_horizon cells are the same); what differs is the side of the
centred target crop, which follows this model's rule: three stride-2 convolutions, three transposed ones, and the loss drops
the prediction's last row and column (128 -> 64, as in notebook 12, but 42 -> 20 where notebook 12's rule gives 21).  The
batch keeps the notebook's three keys: HISTORICAL_SAT_IMAGES [B, 4, S, S] f32, FORECAST_HORIZON [B] f32, TARGET_SAT_IMAGE [B,
s, s] f32 with s = target_side(S)."""
from functools import partial

from ..models.conv3d.nb08_hist_depth import target_side
from .nb10_datamodule import make_fake_batch
from .nb12_datamodule import (Nb12DataModule, make_fake_super_batch, normalise_forecast_horizon,  # noqa: F401
                               super_batch_to_example)

make_fake_nb08_batch = partial(make_fake_batch, side_rule=target_side, horizon_form=normalise_forecast_horizon)


class Nb08DataModule(Nb12DataModule):
    """Nb12DataModule's seeded batches (same super-batches, same draws, same horizon) with notebook 08's target side."""

    make_batch = staticmethod(make_fake_nb08_batch)
