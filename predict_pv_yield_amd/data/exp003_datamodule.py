"""DataModule for the dict batches of experiments/003_perceiver_processes_single_sat_image_then_rnn.py (synthetic: the
experiment's own loaders read the OCF zarr stores, outside the hot path): data/seeded.py over FakeExp003Dataset."""
from ..models.perceiver.exp003 import FakeExp003Dataset
from .seeded import SeededBatchDataModule


class Exp003DataModule(SeededBatchDataModule):
    dataset = FakeExp003Dataset
