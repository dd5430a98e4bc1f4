"""The model-level checks of the notebook frame predictors (models/conv2d/nb*.py, models/conv3d/nb*.py), each stated once, and
one record per notebook holding what differs between them.  tests/test_gpu_notebook_models.py runs every check on the cases
that have it; tests/test_gpu_nbXX.py keep the kernel-level tests.  The float64 CPU restatements are tests/nbXX_reference.py.

Which case has which check (recorded from the per-notebook files this module replaced; `-` is a gap nobody decided on, left
for a change of its own; tests/test_notebook_model_table_cpu.py pins the table):

    check                 nb05      nb07   nb08   nb09   nb10   nb12   nb15   nb16
    golden                a b +f64  a b    a b    a b    a b    a b    a b*   a b*      * case b stores no step3 entries
    full_size             2 sizes   2      2      1 (h)  1 (h)  1      2      2         (h) with the record's horizons
    batch_of_one          (full)    yes    yes    -      -      -      -      -         nb05's B = 1 is a full_size case
    deterministic         a b       yes    yes    -      -      -      yes    yes       nb05 trains on the golden batches
    replay                a b, 5    5      5      3      3      3      5      5         steps replayed after the 2 warm-ups
    fit (checkpoint)      -         yes    yes    -      -      -      yes    yes
    graph_fit             -         +3     +3     +2     +2     +2     +3     +3        batches beyond Trainer's eager steps

Parameters after three Adam steps against the golden: Adam's step is lr * m / (sqrt(v) + eps), about lr per step whatever the
gradient's size.  Where |g| >> eps the step depends on the gradient only through ratios between steps, so a relative gradient
error d moves it by about lr * d: with d <= 1e-2 (ROUTED_TOL's order, the loosest gradient bound here) that is lr * 1e-2, which
99 % of the (stored) entries of every tensor must meet.  The remaining entries are those whose gradient is ~ 0 and may take
either sign in two correct implementations: they may differ by 2 * lr per step, 3 * 2 * lr (+ 1e-6) in all.  The fixture's
parameters must have moved by a tenth of lr at the median, or the comparison shows nothing.  ADAM_BOUNDS holds the three
figures for the two learning rates the notebooks use."""
import importlib
from typing import Callable, NamedTuple, Optional

import numpy as np
import torch

from conv2d_f32_helpers import NORM_TOL, ROOT, _rel, _to

# lr -> (least median movement of the golden's parameters, 99th percentile of |error|, largest |error|)
ADAM_BOUNDS = {1e-3: (1e-4, 1e-5, 3 * 2e-3 + 1e-6), 1e-4: (1e-5, 1e-6, 3 * 2e-4 + 1e-6)}
SAT = ("HISTORICAL_SAT_IMAGES", "FORECAST_HORIZON", "TARGET_SAT_IMAGE")
WB = ("weight", "bias")
ENC_DEC_KEYS = [f"{part}_conv.{i}.{w}" for part in ("encoder", "decoder") for i in (0, 2, 4) for w in WB]


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def _counts(g, n, h, w, integer_flow=False):
    hist = torch.randint(0, 1024, (n, 4, h, w), generator=g).to(torch.int16)
    flow = torch.randint(0, 1024, (n, h, w), generator=g).float()
    if not integer_flow:
        flow = flow + torch.rand(n, h, w, generator=g) * 0.5
    return hist, flow, _randn(g, n)


_half = lambda s: (s - 1) // 2 + 1      # noqa: E731


# ---- the batch builders: (seed, batch, image side) -> a CPU batch ---------------------------------------------------------
def _frames_batch(target_side):
    def build(seed, b, s):
        g, t = _g(seed), target_side(s)
        return dict(zip(SAT, (_randn(g, b, 4, s, s), _randn(g, b), _randn(g, b, t, t))))
    return build


def _stripe_batch(target_side):
    def build(seed, b, s):
        g = _g(seed)
        return dict(zip(SAT, (_randn(g, b, 4, s, s), torch.randint(1, 24, (b,), generator=g),
                              _randn(g, b, target_side(s), target_side(s)))))
    return build


def _nb12_batch(seed, b, s):
    g = _g(seed)
    normalise = importlib.import_module("nb12_reference").G.normalise_forecast_horizon
    horizon = torch.tensor([float(normalise(int(t))) for t in torch.randint(1, 25, (b,), generator=g)])
    return dict(zip(SAT, (_randn(g, b, 4, s, s), horizon, _randn(g, b, _half(s), _half(s)))))


def _counts_batch(target_side):
    def build(seed, b, s):
        g = _g(seed)
        hist, flow, hor = _counts(g, b, s, s)
        t = target_side(s)
        return {"HISTORICAL_SAT_IMAGES": hist, "OPTICAL_FLOW_PREDICTIONS": flow, "FORECAST_HORIZON": hor,
                "TARGET_SAT_IMAGE": torch.randint(0, 1024, (b, t, t), generator=g).to(torch.int16)}
    return build


def _nb05_batch(seed, b, s):
    g = _g(seed)
    return {"input_images": _randn(g, b, 1, s, s), "T0_IMAGES": _randn(g, b, 1, s, s),
            "optical_flow": _randn(g, b, 1, 2, s, s, scale=3.0), "forecast_horizon": _randn(g, b),
            "target_images": _randn(g, b, 1, s, s)}


def _model_target_side(module):
    return lambda s: importlib.import_module(module).target_side(s)


# ---- assertions one notebook only makes -------------------------------------------------------------------------------------
def _nb05_field_without_its_singleton_axis(model, dbatch, y_hat):
    assert torch.equal(y_hat, model({**dbatch, "optical_flow": dbatch["optical_flow"].squeeze(1)}))


def _sat_fit_batch(batch):
    assert tuple(batch["HISTORICAL_SAT_IMAGES"].shape) == (4, 4, 128, 128) and tuple(batch["TARGET_SAT_IMAGE"].shape) == (4, 64, 64)
    assert batch["FORECAST_HORIZON"].dtype == torch.float32


def _counts_fit_batch(batch):
    assert batch["HISTORICAL_SAT_IMAGES"].dtype == torch.int16 and tuple(batch["HISTORICAL_SAT_IMAGES"].shape) == (4, 4, 128, 128)
    assert batch["OPTICAL_FLOW_PREDICTIONS"].dtype == torch.float32 and tuple(batch["TARGET_SAT_IMAGE"].shape) == (4, 64, 64)
    assert float(batch["HISTORICAL_SAT_IMAGES"].float().max()) > 10.0          # raw counts, not normalised


# ---- the record -----------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    model: str                                  # module of LitAutoEncoder, imported when a check runs
    full_batch: Callable                        # (seed, batch, side) -> CPU batch
    full_sizes: tuple                           # ((batch, side, y_hat's shape), ...): the first is the training size
    replay_steps: int                           # steps compared after GraphedTrainStep's two warm-up steps
    target: str = "TARGET_SAT_IMAGE"
    lr: float = 1e-3
    routed: Optional[str] = None                # prefix of the parameters below a pool: their gradients to R.ROUTED_TOL
    step3_tags: tuple = ("a", "b")              # golden cases that store the parameters after three steps
    float64_grads: bool = False                 # first-step loss and gradients against float64 as well as the golden
    horizons: Optional[tuple] = None            # FORECAST_HORIZON of the full-size batch: a float one, one past the image
    full_extra: Optional[Callable] = None       # (model, device batch, y_hat): a full-size assertion of this notebook's own
    batch_of_one: Optional[tuple] = None        # (side, y_hat's shape)
    deterministic: Optional[str] = None         # "drawn": three drawn batches; "golden": the golden batch, per case
    replay_from_golden: bool = False            # initial state and first batch from the golden, two redraws of its shape
    datamodule: Optional[str] = None            # "module:Class" under predict_pv_yield_amd.data
    dm_args: dict = {}
    fit_batch: Optional[Callable] = None        # the checkpoint fit's assertions on a training batch; None: no such check
    state_keys: Optional[list] = None           # the checkpoint's state_dict keys, in order
    graph_fit_extra: Optional[int] = None       # training batches beyond Trainer.GRAPH_EAGER_STEPS; None: no such check

    @property
    def R(self):
        return importlib.import_module(f"{self.name}_reference")

    @property
    def golden(self):
        return f"{ROOT}/tests/golden/{self.name}_small.npz"

    def model_cls(self):
        return importlib.import_module(self.model).LitAutoEncoder

    def dm_cls(self):
        module, cls = self.datamodule.split(":")
        return getattr(importlib.import_module(f"predict_pv_yield_amd.data.{module}"), cls)

    def checks(self):
        """The checks this case has, by the name of the check_* function."""
        have = {"golden": True, "full_size": True, "batch_of_one": self.batch_of_one, "deterministic": self.deterministic,
                "replay": True, "fit": self.fit_batch, "graph_fit": self.graph_fit_extra}
        return {k for k, v in have.items() if v}


M2, M3 = "predict_pv_yield_amd.models.conv2d.", "predict_pv_yield_amd.models.conv3d."
DM4 = dict(batch_size=4, n_val_data=1, n_super_batches=1)
DM2 = dict(batch_size=2, n_val_data=1, n_super_batches=1, n_timesteps=12)

CASES = {c.name: c for c in (
    Case("nb05", M2 + "nb05_more_inputs", _nb05_batch, ((10, 64, (10, 1, 64, 64)), (1, 7, (1, 1, 7, 7))), 5,
         target="target_images", float64_grads=True, full_extra=_nb05_field_without_its_singleton_axis,
         deterministic="golden", replay_from_golden=True),
    Case("nb07", M2 + "nb07_multi_hist", _frames_batch(_model_target_side(M2 + "nb07_multi_hist")),
         ((4, 128, (4, 1, 65, 65)), (2, 15, (2, 1, 9, 9))), 5, batch_of_one=(31, (1, 1, 17, 17)), deterministic="drawn",
         datamodule="nb08_datamodule:Nb08DataModule", dm_args=DM4, fit_batch=_sat_fit_batch, state_keys=ENC_DEC_KEYS,
         graph_fit_extra=3),
    Case("nb08", M3 + "nb08_hist_depth", _frames_batch(_model_target_side(M3 + "nb08_hist_depth")),
         ((4, 128, (4, 1, 65, 65)), (2, 15, (2, 1, 9, 9))), 5, batch_of_one=(31, (1, 1, 17, 17)), deterministic="drawn",
         datamodule="nb08_datamodule:Nb08DataModule", dm_args=DM4, fit_batch=_sat_fit_batch, state_keys=ENC_DEC_KEYS,
         graph_fit_extra=3),
    Case("nb09", M2 + "nb09_stripe_ae", _stripe_batch(lambda s: 64), ((2, 128, (2, 1, 65, 65)),), 3, horizons=(7.9, 26.0),
         datamodule="nb10_datamodule:Nb10DataModule", dm_args=DM2, graph_fit_extra=2),
    Case("nb10", M2 + "nb10_just_conv", _stripe_batch(_half), ((2, 128, (2, 1, 64, 64)),), 3, horizons=(7.9, 25.0),
         datamodule="nb10_datamodule:Nb10DataModule", dm_args=DM2, graph_fit_extra=2),
    Case("nb12", M3 + "nb12_just_3d_conv", _nb12_batch, ((2, 128, (2, 1, 1, 64, 64)),), 3, lr=1e-4,
         datamodule="nb12_datamodule:Nb12DataModule", dm_args=DM2, graph_fit_extra=2),
    Case("nb15", M2 + "nb15_strided_ae", _counts_batch(_model_target_side(M2 + "nb15_strided_ae")),
         ((4, 128, (4, 1, 63, 63)), (2, 31, (2, 1, 15, 15))), 5, step3_tags=("a",), deterministic="drawn",
         datamodule="nb15_datamodule:Nb15DataModule", dm_args=DM4, fit_batch=_counts_fit_batch,
         state_keys=[f"conv.{i}.{w}" for i in (0, 2, 4, 6, 8, 10, 12) for w in WB], graph_fit_extra=3),
    Case("nb16", M2 + "nb16_maxpool", _counts_batch(lambda s: (s - 8) // 3 + 24),
         ((4, 128, (4, 1, 48, 48)), (2, 11, (2, 1, 9, 9))), 5, routed="encoder", step3_tags=("a",),
         deterministic="drawn", datamodule="nb16_datamodule:Nb16DataModule", dm_args=DM4, fit_batch=_counts_fit_batch,
         state_keys=[f"{part}_conv{i}.{w}" for part in ("encoder", "decoder") for i in (1, 2, 3, 4) for w in WB],
         graph_fit_extra=3),
)}


# ---- the golden's entries: whole tensors, or the sampled entries of notebooks 09 / 10 / 12 ------------------------------------
def golden_case(R, gold, tag):
    """(batch, initial state_dict) of golden case `tag`: read from the fixture or redrawn from the seeds its maker used."""
    return R.golden_case(gold, tag) if hasattr(R, "golden_case") else (R.G.draw_batch(tag), R.G.draw_parameters())


def stored(R, name, t):
    """The entries of t the golden stores under `name` as float64: R.stored's sample, or the whole tensor."""
    return R.stored(name, t)[0] if hasattr(R, "stored") else torch.as_tensor(t).detach().cpu().double()


def check_stored(R, gold, name, t, tol, entries_only=False):
    """t against golden entry `name` to relative norm tol (R.check_stored: a sampled tensor's norm and sum as well); for a
    tensor stored whole that is _rel(t, gold[name]) <= tol.  Returns the error; entries_only: without asserting."""
    if hasattr(R, "check_stored"):
        return R.check_stored(gold, name, t, tol, entries_only=entries_only)
    err = _rel(t, gold[name])
    assert entries_only or err <= tol, (name, err)
    return err


def check_adam_steps(R, gold, tag, init, params, lr):
    """`params` ((name, tensor) pairs) after three Adam steps from `init` against the golden's step3 entries: ADAM_BOUNDS."""
    least_moved, q99_bound, worst_bound = ADAM_BOUNDS[lr]
    for k, p in params:
        name = f"{tag}/step3/{k}"
        got, first = stored(R, name, p), stored(R, name, init[k])
        want = torch.from_numpy(gold[name]).double().reshape(got.shape)
        err, moved = (got - want).abs(), (want - first).abs()
        q99 = err.flatten().sort().values[int(0.99 * (err.numel() - 1))].item()
        print(f"{tag} step3 {k}: max {err.max().item():.3e} 99% {q99:.3e} moved median {moved.median().item():.3e}")
        assert moved.median().item() >= least_moved, k       # the fixture's parameters did move (three steps of lr)
        assert q99 <= q99_bound, (k, q99)
        assert err.max().item() <= worst_bound, k


def check_fit64(R, gold, tag, batch, target):
    """CPU: three float64 Adam steps of the reference land where the notebook's float32 ones did (the maker's check_fit,
    restated): every loss to 1e-5, 99 % of every parameter's entries within the maker's FIT_Q99."""
    p = R.params64(R.G.draw_parameters())
    opt = torch.optim.Adam(list(p.values()), lr=R.G.LR)
    for want in gold[f"{tag}/losses"]:
        opt.zero_grad()
        loss = R.loss64(R.forward64(p, batch), batch[target])
        assert abs(loss.item() - want) <= 1e-5 * want
        loss.backward()
        opt.step()
    for k, v in p.items():
        err = (v.detach() - torch.from_numpy(gold[f"{tag}/step3/{k}"]).double()).abs().flatten().sort().values
        assert err[int(0.99 * (err.numel() - 1))].item() <= R.G.FIT_Q99, k


# ---- the checks -----------------------------------------------------------------------------------------------------------
def _fresh(case, device, seed):
    torch.manual_seed(seed)
    return case.model_cls()().to(device)


def _loaded(case, device, init):
    model = case.model_cls()()
    model.load_state_dict(init)
    return model.to(device)


def _train(model, opt, batch):
    opt.zero_grad(set_to_none=True)
    loss = model.training_step(batch, 0)
    loss.backward()
    opt.step()
    return loss


def check_model_against_golden(device, case, tag):
    """Forward, first-step gradients, three losses and the parameters after three Adam steps against the golden fixture."""
    R, gold = case.R, np.load(case.golden)
    batch, init = golden_case(R, gold, tag)
    model = _loaded(case, device, init)
    dbatch = _to(batch, device)
    y_hat = model(dbatch)
    assert tuple(y_hat.shape) == tuple(gold[f"{tag}/y_hat"].shape)
    check_stored(R, gold, f"{tag}/y_hat", y_hat, NORM_TOL)
    if case.float64_grads:
        p64 = R.params64(init)
        y64 = R.forward64(p64, batch)
        assert _rel(y_hat.detach(), y64.detach()) <= NORM_TOL
        loss64 = R.loss64(y64, batch[case.target])
        loss64.backward()
    opt = model.configure_optimizers()
    assert opt.param_groups[0]["lr"] == case.lr
    losses = []
    for step in range(3):
        opt.zero_grad(set_to_none=True)
        loss = model.training_step(dbatch, 0)
        loss.backward()
        if step == 0:
            tol = {k: R.ROUTED_TOL if case.routed and k.startswith(case.routed) else NORM_TOL
                   for k, _ in model.named_parameters()}
            for k, p in model.named_parameters():       # every figure first, then the assertions
                err = check_stored(R, gold, f"{tag}/grad/{k}", p.grad, tol[k], entries_only=True)
                print(f"{tag} grad {k}: rel {err:.3e} (bound {tol[k]})")
            for k, p in model.named_parameters():
                check_stored(R, gold, f"{tag}/grad/{k}", p.grad, tol[k])
            if case.float64_grads:
                assert abs(loss.item() - loss64.item()) <= 1e-5 * loss64.item(), (loss.item(), loss64.item())
                for k, p in model.named_parameters():
                    err = _rel(p.grad, p64[k].grad)
                    assert err <= NORM_TOL, (k, err, "against float64")
        opt.step()
        losses.append(loss.item())
    for got, want in zip(losses, gold[f"{tag}/losses"]):
        assert abs(got - want) <= 1e-5 * want, (losses, gold[f"{tag}/losses"])
    if tag in case.step3_tags:                  # the other cases store losses only after the first step (fixture size)
        check_adam_steps(R, gold, tag, init, list(model.named_parameters()), case.lr)


def check_full_size_forward_and_loss(device, case, b, s, shape):
    """A drawn batch at the notebook's size, or the smallest the model takes, against float64."""
    R = case.R
    model = _fresh(case, device, 5)
    batch = case.full_batch(50, b, s)
    if case.horizons is not None:
        batch["FORECAST_HORIZON"] = torch.tensor(case.horizons)
    dbatch = _to(batch, device)
    y_hat = model(dbatch)
    assert tuple(y_hat.shape) == shape
    if case.full_extra is not None:
        case.full_extra(model, dbatch, y_hat)
    loss = model.training_step(dbatch, 0)
    y64 = R.forward64(R.params64(model.state_dict(), requires_grad=False), batch)
    assert _rel(y_hat.detach(), y64) <= NORM_TOL
    ref = R.loss64(y64, batch[case.target]).item()
    assert abs(loss.item() - ref) <= 1e-5 * ref, (loss.item(), ref)


def check_batch_of_one(device, case):
    """The batch axis survives B = 1 (a notebook's squeeze() would drop it)."""
    side, shape = case.batch_of_one
    model = _fresh(case, device, 6)
    batch = _to(case.full_batch(51, 1, side), device)
    assert tuple(model(batch).shape) == shape
    assert torch.isfinite(model.training_step(batch, 0))


def check_two_eager_runs_are_equal_bit_for_bit(device, case, tag=None):
    """Three training steps twice from one state: equal losses as floats, torch.equal parameters."""
    b, s, _ = case.full_sizes[0]

    def run():
        if case.deterministic == "golden":
            batch, init = golden_case(case.R, None, tag)
            model, batches = _loaded(case, device, init), [_to(batch, device)] * 3
        else:
            model, batches = _fresh(case, device, 3), [_to(case.full_batch(60 + i, b, s), device) for i in range(3)]
        opt = model.configure_optimizers()
        return model, [_train(model, opt, batch).item() for batch in batches]

    (m1, l1), (m2, l2) = run(), run()
    assert l1 == l2
    for (k, p), q in zip(m1.named_parameters(), m2.parameters()):
        assert torch.equal(p, q), k


def check_train_step_replays_as_a_hip_graph(device, case, tag=None):
    """case.replay_steps steps through GraphedTrainStep, cycling three batches: every loss == the eager step's as floats, the
    parameters torch.equal after the warm-up steps and at the end."""
    from predict_pv_yield_amd.graphs import GraphedTrainStep
    from predict_pv_yield_amd.optim import HipAdam
    if case.replay_from_golden:     # the replay reads what is copied into the captured batch: two more of the golden's shape
        batch, init = golden_case(case.R, None, tag)
        batches = [_to(batch, device)] + [_to(case.R.G.draw_batch(tag, seed=2000 + i), device) for i in range(2)]
        make = lambda: _loaded(case, device, init)      # noqa: E731
    else:
        b, s, _ = case.full_sizes[0]
        batches = [_to(case.full_batch(70 + i, b, s), device) for i in range(3)]
        make = lambda: _fresh(case, device, 11)      # noqa: E731
    model_e, model_g = make(), make()
    opt_e = HipAdam(model_e.parameters(), lr=case.lr, capturable=False)
    opt_g = HipAdam(model_g.parameters(), lr=case.lr, capturable=True)
    step = GraphedTrainStep(model_g, opt_g, batches[0], warmup=2)
    try:
        for _ in range(2):                      # the warm-up steps are training steps: the eager model takes them too
            _train(model_e, opt_e, batches[0])
        for p, q in zip(model_g.parameters(), model_e.parameters()):
            assert torch.equal(p, q)
        for i in range(case.replay_steps):
            loss = _train(model_e, opt_e, batches[i % 3])
            assert float(step(batches[i % 3])) == float(loss), f"step {i}"
        for p, q in zip(model_g.parameters(), model_e.parameters()):
            assert torch.equal(p, q)
    finally:
        step.close()


def check_trainer_fit_on_the_fake_datamodule(device, case, tmp_path):
    """Trainer.fit for an epoch of three batches, the logged losses, and the checkpoint's round trip."""
    from predict_pv_yield_amd import lightning as pl
    LitAutoEncoder = case.model_cls()

    class Recording(LitAutoEncoder):
        seen = []

        def log_dict(self, d, **kw):
            type(self).seen.extend((k, v.detach()) for k, v in d.items())
            return super().log_dict(d, **kw)

    torch.manual_seed(1)
    model = Recording()
    dm = case.dm_cls()(n_train_data=3, **case.dm_args)
    ckpt = pl.ModelCheckpoint(save_last=True, dirpath=str(tmp_path / "ck"))
    trainer = pl.Trainer(gpus=1, max_epochs=1, callbacks=[ckpt], log_every_n_steps=1)
    trainer.fit(model, datamodule=dm)
    case.fit_batch(next(iter(dm.train_dataloader())))
    train = [float(v) for k, v in Recording.seen if k == "Loss/Train"]
    assert len(train) == 3 and all(np.isfinite(train)), train
    assert any(k == "Loss/Validation" for k, _ in Recording.seen)
    state = torch.load(ckpt.last_model_path)["state_dict"]
    assert list(state) == case.state_keys
    fresh = LitAutoEncoder()
    fresh.load_state_dict(state)
    for (k, p), q in zip(model.state_dict().items(), fresh.state_dict().values()):
        assert torch.equal(p.cpu(), q), k


def check_trainer_fit_with_hip_graph_matches_the_eager_fit(device, case):
    """`run.py ... +trainer.hip_graph=true`: Trainer(hip_graph=True) replays the step after its eager steps; more batches
    than those, same parameters and logged losses as the eager fit."""
    from predict_pv_yield_amd import lightning as pl
    dm = case.dm_cls()(n_train_data=pl.Trainer.GRAPH_EAGER_STEPS + case.graph_fit_extra, **case.dm_args)
    results = []
    for graph in (False, True):
        torch.manual_seed(2)
        model = case.model_cls()()
        trainer = pl.Trainer(gpus=1, max_epochs=1, hip_graph=graph, log_every_n_steps=1)
        trainer.fit(model, datamodule=dm)
        results.append(({k: v.detach().clone() for k, v in model.state_dict().items()}, dict(trainer.callback_metrics)))
    (sd_e, log_e), (sd_g, log_g) = results
    for k in sd_e:
        assert torch.equal(sd_e[k], sd_g[k]), k
    assert np.isfinite(float(log_g["Loss/Train_epoch"])) and float(log_g["Loss/Train_epoch"]) == float(log_e["Loss/Train_epoch"])
