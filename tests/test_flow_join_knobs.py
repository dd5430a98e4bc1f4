"""CPU: the `future_frames` / `flow_channel` knobs of the six satellite models that read frames past t0 (the reference's
`# TODO: Use optical flow, not actual sat images of the future!`) and the three configs that switch them on.  Construction
only: the join itself runs on the MI355X (tests/test_gpu_flow_join_models.py)."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _classes():
    from predict_pv_yield_amd.models.conv2d.exp002 import LitModel as Exp002
    from predict_pv_yield_amd.models.conv3d.model_sat_nwp import Model as SatNwp
    from predict_pv_yield_amd.models.perceiver.exp003 import LitModel as Exp003
    from predict_pv_yield_amd.models.perceiver.perceiver import PerceiverModel
    from predict_pv_yield_amd.models.perceiver.perceiver_conv3d_nwp_sat import Model as PerceiverConv3d
    from predict_pv_yield_amd.models.perceiver.perceiver_nwp_sat import Model as PerceiverNwpSat
    small = dict(history_minutes=10, forecast_minutes=10)
    return {
        "model_sat_nwp": (SatNwp, dict(small, number_of_conv3d_layers=2, image_size_pixels=8, nwp_image_size_pixels=8,
                                       fc1_output_features=8, fc2_output_features=8, fc3_output_features=8)),
        "perceiver": (PerceiverModel, dict(small, num_latents=8, latent_dim=8)),
        "perceiver_nwp_sat": (PerceiverNwpSat, dict(small, num_latents=8, latent_dim=8)),
        "perceiver_conv3d_nwp_sat": (PerceiverConv3d, dict(small, num_latents=8, latent_dim=8)),
        "exp002": (Exp002, dict(history_len=2, forecast_len=2)),
        "exp003": (Exp003, dict(history_len=2, forecast_len=2)),
    }


NAMES = ["model_sat_nwp", "perceiver", "perceiver_nwp_sat", "perceiver_conv3d_nwp_sat", "exp002", "exp003"]


@pytest.mark.parametrize("name", NAMES)
def test_model_takes_and_stores_the_knobs(name):
    cls, kw = _classes()[name]
    model = cls(**kw, future_frames="optical_flow", flow_channel=0)
    assert model.future_frames == "optical_flow" and model.flow_channel == 0
    plain = cls(**kw)
    assert plain.future_frames == "true" and plain.flow_channel is None
    per_channel = cls(**kw, future_frames="optical_flow")
    assert per_channel.future_frames == "optical_flow" and per_channel.flow_channel is None


@pytest.mark.parametrize("name", NAMES)
def test_model_rejects_other_values(name):
    cls, kw = _classes()[name]
    with pytest.raises(ValueError, match="future_frames"):
        cls(**kw, future_frames="flow")
    with pytest.raises(ValueError, match="flow_channel"):
        cls(**kw, future_frames="optical_flow", flow_channel=-1)
    with pytest.raises(ValueError, match="flow_channel"):
        cls(**kw, future_frames="optical_flow", flow_channel="HRV")


@pytest.mark.parametrize("name", NAMES)
def test_the_knobs_are_attributes_not_state(name):
    cls, kw = _classes()[name]
    with_knob = cls(**kw, future_frames="optical_flow", flow_channel=0)
    without = cls(**kw)
    assert list(with_knob.state_dict().keys()) == list(without.state_dict().keys())
    assert [n for n, _ in with_knob.named_buffers()] == [n for n, _ in without.named_buffers()]
    without.load_state_dict(with_knob.state_dict())


@pytest.mark.parametrize("model,datamodule,target,kwargs", [
    ("exp003_perceiver_optical_flow", "exp003_fake", "predict_pv_yield_amd.models.perceiver.exp003.LitModel",
     dict(history_len=6, forecast_len=12, operand_dtype="bf16", future_frames="optical_flow", flow_channel=0)),
    ("exp002_cnn_rnn_optical_flow", "exp002_fake", "predict_pv_yield_amd.models.conv2d.exp002.LitModel",
     dict(history_len=6, forecast_len=12, future_frames="optical_flow", flow_channel=0)),
    ("conv3d_sat_nwp_optical_flow", "netcdf_datamodule", "predict_pv_yield_amd.models.conv3d.model_sat_nwp.Model",
     dict(forecast_minutes=120, history_minutes=30, number_of_conv3d_layers=6, image_size_pixels=24, number_sat_channels=11,
          include_future_satellite=True, output_variable="gsp_yield", future_frames="optical_flow")),
])
def test_optical_flow_configs_compose(model, datamodule, target, kwargs):
    from predict_pv_yield_amd import hydra_lite as H
    cfg = H.compose(os.path.join(ROOT, "configs"), "config", [f"model={model}", f"datamodule={datamodule}", "callbacks=none"])
    assert cfg.model._target_ == target
    for k, v in kwargs.items():
        assert cfg.model[k] == v, (k, cfg.model[k], v)
    # the new file is the existing one plus the knobs
    base = H.compose(os.path.join(ROOT, "configs"), "config", [f"model={model[:-len('_optical_flow')]}",
                                                               f"datamodule={datamodule}", "callbacks=none"])
    extra = {k: cfg.model[k] for k in cfg.model if k not in base.model}
    assert set(extra) == {"future_frames", "flow_channel"} & set(kwargs)
    assert all(cfg.model[k] == base.model[k] for k in base.model)
    built = H.instantiate(cfg.model)
    assert built.future_frames == "optical_flow" and built.flow_channel == kwargs.get("flow_channel")


def test_sat_nwp_optical_flow_model_composes_with_the_fake_datamodule_of_its_shapes():
    """`run.py model=conv3d_sat_nwp_optical_flow datamodule.data_path=configs/dataset/conv3d_sat_nwp callbacks=none`: the fake
    NetCDF datamodule with the dataset configuration of the sat+NWP model's shapes."""
    from predict_pv_yield_amd import hydra_lite as H
    data_path = os.path.join(ROOT, "configs", "dataset", "conv3d_sat_nwp")
    cfg = H.compose(os.path.join(ROOT, "configs"), "config", ["model=conv3d_sat_nwp_optical_flow", "callbacks=none",
                                                              f"datamodule.data_path={data_path}"])
    assert cfg.model._target_ == "predict_pv_yield_amd.models.conv3d.model_sat_nwp.Model"
    assert cfg.model.future_frames == "optical_flow" and cfg.datamodule.fake_data is True
    assert os.path.exists(os.path.join(cfg.datamodule.data_path, "configuration.yaml"))


def test_graph_capture_is_refused_for_the_in_forward_join():
    """HIP-graph replay of a step that computes the flow in forward() is out of scope: one clear error, before any capture."""
    from predict_pv_yield_amd.models._flow_join import refuse_graph_capture
    cls, kw = _classes()["exp002"]
    refuse_graph_capture(cls(**kw))
    with pytest.raises(RuntimeError, match="HIP-graph replay"):
        refuse_graph_capture(cls(**kw, future_frames="optical_flow"))
