"""The `future_frames` / `flow_channel` knobs of the satellite models that read frames past t0.

The reference hands these models the TRUE future frames and marks it in five places with
`# TODO: Use optical flow, not actual sat images of the future!` (predict_pv_yield/models/perceiver/perceiver.py:118,
perceiver_nwp_sat.py:117, perceiver_conv3d_nwp_sat.py:145, experiments/002_...py:167, experiments/003_...py:155).
future_frames="optical_flow" replaces the future time slices of the batch's satellite tensor by frames advected from the
observed ones (optical_flow.replace_future_frames_with_flow) before anything else reads them.  Both knobs are plain
attributes: no parameter, no buffer, state_dict keys stay the reference's.
"""
from typing import Optional

import torch

FUTURE_FRAMES = ("true", "optical_flow")


def check_knobs(future_frames: str, flow_channel: Optional[int]) -> None:
    if future_frames not in FUTURE_FRAMES:
        raise ValueError("future_frames must be 'true' or 'optical_flow'")
    if flow_channel is not None and (isinstance(flow_channel, bool) or not isinstance(flow_channel, int) or flow_channel < 0):
        raise ValueError("flow_channel must be None (each channel along its own flow) or the index of the channel the "
                         "shared flow is estimated on")


def joined_frames(model, sat: torch.Tensor, n_future: int, layout: str, source: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`sat` (f32, NCTHW or NTHWC) as the model is to see it: unchanged for future_frames="true" and for a tensor a loader
    has tagged `_pv_advected` (the tag is looked up on `source`, the batch's own tensor, when `sat` is a slice or a cast of
    it); otherwise its last n_future time slices advected."""
    if model.future_frames != "optical_flow" or getattr(sat if source is None else source, "_pv_advected", False):
        return sat
    from ..optical_flow import replace_future_frames_with_flow
    return replace_future_frames_with_flow(sat.float(), n_future=n_future, layout=layout, flow_channel=model.flow_channel)


def refuse_graph_capture(model) -> None:
    """HIP-graph replay of a train step that computes the flow inside forward() is out of scope: one clear error before any
    capture (graphs.GraphedTrainStep, Trainer(hip_graph=True)) instead of a graph nobody has verified."""
    if getattr(model, "flow_join_in_forward", False) and getattr(model, "future_frames", "true") == "optical_flow":
        raise RuntimeError(f"{type(model).__module__}.{type(model).__name__}(future_frames='optical_flow') computes the "
                           "Farnebäck flow inside forward(); HIP-graph replay of that step is not supported: train with "
                           "hip_graph=False (or future_frames='true')")
