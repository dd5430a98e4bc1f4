"""What the notebook frame predictors' LitAutoEncoders (notebooks 05, 07, 08, 09, 10, 12, 15, 16) share: the checks of a batch's
tensors, the train / validation step with its logging, and the optimiser.  A model file keeps its layers, its side rule
(output_side, target_side), the call into its chain builder and its loss line.

Every model checks in the same order: shapes first, then the device, then the sides, so a mis-shaped batch is refused with
a ValueError wherever it lies."""
import torch

from .. import lightning as pl
from .conv3d.flow_autoencoder import FORECAST_HORIZON, HISTORICAL_SAT_IMAGES, OPTICAL_FLOW_PREDICTIONS, TARGET_SAT_IMAGE

N_HIST_IMAGES = 4


def check_target_side(nb, side_rule, image_shape, target_shape, note=lambda want: "") -> None:
    """image_shape: (H, W) of the history images; the target must be [B, side_rule(H), side_rule(W)].  note(want): a clause
    on how the target lines up with the output, for the message."""
    want = tuple(side_rule(int(side)) for side in image_shape)
    if len(target_shape) != 3 or tuple(target_shape[1:]) != want:
        raise ValueError(f"{nb} LitAutoEncoder: TARGET_SAT_IMAGE must be [B, {want[0]}, {want[1]}] for {image_shape[0]} x "
                         f"{image_shape[1]}-pixel inputs{note(want)}, got {tuple(target_shape)}")


def _require_device(*tensors):
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError("predict_pv_yield_amd LitAutoEncoder runs on the MI355X only: move the module and the "
                           "batch to cuda (there is no CPU fallback)")


class NotebookAutoEncoder(pl.LightningModule):
    """A subclass sets nb ("nb09"), output_side and check_target_side (its module's functions, as staticmethods), builds its
    layers, and defines forward(x) and loss(y_hat, y)."""
    nb = None
    lr = 0.001
    # the batch keys of the image whose sides set the target's, and of the target (notebook 05 spells them differently)
    image_key, target_key = HISTORICAL_SAT_IMAGES, TARGET_SAT_IMAGE

    def history_and_horizon(self, x, horizon_dtype=None):
        """(history [B, 4, H, W] as float32, horizon [B] on its device, cast to horizon_dtype if given) of a batch whose horizon
        the first layer's kernels turn into an input channel."""
        hist_images, horizon = x[HISTORICAL_SAT_IMAGES], x[FORECAST_HORIZON]
        if hist_images.dim() != 4 or hist_images.shape[1] != N_HIST_IMAGES:
            raise ValueError(f"{self.nb} LitAutoEncoder takes HISTORICAL_SAT_IMAGES [B, {N_HIST_IMAGES}, H, W], got "
                             f"{tuple(hist_images.shape)}")
        if horizon.numel() != hist_images.shape[0]:       # a shape like the one above: refused before the device is looked at
            raise ValueError(f"{self.nb} LitAutoEncoder takes FORECAST_HORIZON [B], got {tuple(horizon.shape)} for "
                             f"{hist_images.shape[0]} examples")
        _require_device(hist_images)
        for side in hist_images.shape[2:]:
            self.output_side(int(side))
        return hist_images.float(), horizon.to(device=hist_images.device, dtype=horizon_dtype).reshape(-1)

    def counts_and_horizon(self, x):
        """(history [B, 4, S, S], flow prediction [B, S, S], horizon [B] f32) of a batch of raw counts, which stay int16 /
        float32: the first layer normalises them while it stages its input."""
        history, flow_pred, horizon = x[HISTORICAL_SAT_IMAGES], x[OPTICAL_FLOW_PREDICTIONS], x[FORECAST_HORIZON]
        if (history.dim() != 4 or history.shape[1] != N_HIST_IMAGES
                or tuple(flow_pred.shape) != (history.shape[0],) + tuple(history.shape[2:])):
            raise ValueError(f"{self.nb} LitAutoEncoder takes HISTORICAL_SAT_IMAGES [B, 4, S, S] and OPTICAL_FLOW_PREDICTIONS "
                             f"[B, S, S], got {tuple(history.shape)} / {tuple(flow_pred.shape)}")
        _require_device(history, flow_pred)
        for side in history.shape[2:]:
            self.output_side(int(side))
        history, flow_pred = (self.counts(t) for t in (history, flow_pred))
        return history, flow_pred, horizon.to(device=history.device, dtype=torch.float32).reshape(-1)

    def flow_inputs_and_horizon(self, x, flow_pred_key, t0_key, flow_field_key, horizon_key):
        """(flow prediction [B, H, W], t0 image [B, H, W], flow field [B, 2, H, W], horizon [B]), all float32, of a batch whose
        flow prediction and t0 image are [B, 1, H, W] and whose flow field is [B, 1, 2, H, W] or [B, 2, H, W] (planar, x then
        y).  The singleton axes are dropped as views and the batch axis survives B = 1."""
        flow_pred, t0, field, horizon = x[flow_pred_key], x[t0_key], x[flow_field_key], x[horizon_key]
        if flow_pred.dim() != 4 or flow_pred.shape[1] != 1 or tuple(t0.shape) != tuple(flow_pred.shape):
            raise ValueError(f"{self.nb} LitAutoEncoder takes {flow_pred_key} and {t0_key} [B, 1, H, W], got "
                             f"{tuple(flow_pred.shape)} / {tuple(t0.shape)}")
        b, _, h, w = flow_pred.shape
        if tuple(field.shape) not in ((b, 1, 2, h, w), (b, 2, h, w)):
            raise ValueError(f"{self.nb} LitAutoEncoder takes {flow_field_key} [B, 1, 2, H, W] or [B, 2, H, W] = "
                             f"[{b}, (1,) 2, {h}, {w}], got {tuple(field.shape)}")
        if horizon.numel() != b:
            raise ValueError(f"{self.nb} LitAutoEncoder takes {horizon_key} [B], got {tuple(horizon.shape)} for {b} examples")
        _require_device(flow_pred, t0, field)
        for side in (h, w):
            self.output_side(int(side))
        return (flow_pred.float().reshape(b, h, w), t0.float().reshape(b, h, w), field.float().reshape(b, 2, h, w),
                horizon.to(device=flow_pred.device, dtype=torch.float32).reshape(-1))

    @staticmethod
    def counts(t):
        return t if t.dtype in (torch.int16, torch.float32) else t.float()

    def _training_or_validation_step(self, batch, is_train_step):
        y = batch[self.target_key]
        self.check_target_side(tuple(batch[self.image_key].shape[-2:]), y.shape)
        loss = self.loss(self(batch), y)
        tag = "Loss/Train" if is_train_step else "Loss/Validation"
        self.log_dict({tag: loss}, on_step=is_train_step, on_epoch=True)
        return loss

    def training_step(self, batch, batch_idx):
        return self._training_or_validation_step(batch, is_train_step=True)

    def validation_step(self, batch, batch_idx):
        return self._training_or_validation_step(batch, is_train_step=False)

    def configure_optimizers(self):
        from ..optim import HipAdam
        return HipAdam(self.parameters(), lr=self.lr)
