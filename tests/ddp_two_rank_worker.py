"""Worker of tests/test_gpu_ddp.py: one data-parallel rank training the reduced Conv3D model for a few steps in a given
large-gradient mode and saving the consolidated parameters of rank 0.  Either one of two ranks that SHARE the single GPU of
the test box (gloo for the collectives, PV_SINGLE_DEVICE=1; WORLD_SIZE 2 or 8, PV_TEST_GLOBAL_BATCH samples split among them), or the only rank of a one-rank RCCL group
(WORLD_SIZE=1, PV_DIST_SINGLE_RANK=1, backend "nccl": the collectives of the N > 1 path really run through RCCL).
The process group is initialised BEFORE anything touches the GPU.
Usage: python ddp_two_rank_worker.py <mode> <out.pt> <steps>
The modes in CASES instead check the state HipAdam and the Trainer keep around fc1's K-sharded column shard and the operand
copies cached on the parameters (tests/test_gpu_ddp.py); every rank writes its findings (rank r > 0 to <out.pt>.rank<r>)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from predict_pv_yield_amd import distributed as D
from predict_pv_yield_amd._large_param import large_of
from predict_pv_yield_amd.models.conv3d.model import Model
from predict_pv_yield_amd.optim import HipAdam

SMALL = dict(include_pv_yield=False, include_nwp=False, forecast_minutes=60, history_minutes=60,
             number_of_conv3d_layers=4, conv3d_channels=32, image_size_pixels=16, number_sat_channels=11,
             fc1_output_features=16, fc2_output_features=16, fc3_output_features=16)


def _rank_batch(dev, seed, n_global=4, nan=False):
    """This rank's contiguous share of a seeded global batch of the reduced model (nan: every target is NaN, so is every
    rank's loss -- a NaN in the satellite input would not do: the ReLUs of the conv tower map it to 0)."""
    g = torch.Generator().manual_seed(seed)
    sat = torch.randn(n_global, 11, 25, 16, 16, generator=g)
    pv = torch.rand(n_global, 25, 128, generator=g)
    if nan:
        pv.fill_(float("nan"))
    lo, hi = D.shard_range(n_global)
    return {"satellite": {"data": sat[lo:hi].to(dev)}, "pv": {"pv_yield": pv[lo:hi].to(dev)}}


def _ksharded_model(dev, world):
    torch.manual_seed(518)
    model = Model(**SMALL, precision="bf16").to(dev)
    D.broadcast_parameters(model)
    opt = model.configure_optimizers()
    opt.grad_scale = 1.0 / world
    opt.set_large_grad_mode("ksharded")
    assert opt.large_grad_mode == "ksharded", opt.large_grad_mode
    return model, opt, D.OverlappedGradSync(model, large_numel=model.fc1.weight.numel())


def _step(model, opt, sync, batch):
    opt.zero_grad(set_to_none=True)
    loss = model.training_step(batch, 0)
    loss.backward()
    sync.finish()
    opt.step()
    return float(loss.detach())


def _consolidated(model, opt):
    """(state_dict, fc1's exp_avg, exp_avg_sq and step) after consolidate_sharded(), as CPU copies."""
    opt.consolidate_sharded()
    torch.cuda.synchronize()
    st = opt.state[model.fc1.weight]
    return {"state": {k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
            "exp_avg": st["exp_avg"].cpu().clone(), "exp_avg_sq": st["exp_avg_sq"].cpu().clone(), "step": float(st["step"])}


def case_reload(rank, world, dev, out_path):
    """ksharded step 1 -> consolidate -> checkpoint C1 -> step 2 (R1); load C1 into the model and the optimiser -> step 2 again
    (R2); load C1 into the model and a NEW HipAdam set to ksharded -> step 2 (R3).  R2 and R3 must be R1."""
    import copy
    model, opt, sync = _ksharded_model(dev, world)
    b1, b2 = _rank_batch(dev, 7), _rank_batch(dev, 8)
    _step(model, opt, sync, b1)
    opt.consolidate_sharded()
    c1_model = {k: v.detach().clone() for k, v in model.state_dict().items()}
    c1_opt = copy.deepcopy(opt.state_dict())
    out = {}
    out["loss1"] = _step(model, opt, sync, b2)
    out["r1"] = _consolidated(model, opt)
    model.load_state_dict(c1_model)
    opt.load_state_dict(copy.deepcopy(c1_opt))
    out["loss2"] = _step(model, opt, sync, b2)
    out["r2"] = _consolidated(model, opt)
    model.load_state_dict(c1_model)
    opt2 = model.configure_optimizers()          # a second fit / a resume: a new optimiser on the same parameters
    opt2.grad_scale = 1.0 / world
    opt2.load_state_dict(copy.deepcopy(c1_opt))
    opt2.set_large_grad_mode("ksharded")
    out["mode3"] = opt2.large_grad_mode
    out["loss3"] = _step(model, opt2, sync, b2)
    out["r3"] = _consolidated(model, opt2)
    return out


def _mode_probe(model):
    """Trainer callback: the large-gradient mode and whether fc1 carries a shard, at the end of each training epoch."""
    from predict_pv_yield_amd import lightning as pl

    class ModeProbe(pl.Callback):
        seen = []

        def on_train_epoch_end(self, trainer, module):
            self.seen.append((trainer.optimizers[0].large_grad_mode, large_of(model.fc1.weight).kshard is not None))
    return ModeProbe()


def case_after_fit(rank, world, dev, out_path):
    """Trainer(large_grad_mode="ksharded").fit, then fc1's state; the attributes are read BEFORE any forward (with a shard
    left in place a forward would be collective: rank 0 alone would wait for rank 1 forever)."""
    from predict_pv_yield_amd import lightning as pl
    torch.manual_seed(518)
    model = Model(**SMALL, precision="bf16").to(dev)
    probe = _mode_probe(model)
    trainer = pl.Trainer(gpus=1, max_epochs=1, large_grad_mode="ksharded", callbacks=[probe])
    trainer.fit(model, [_rank_batch(dev, s) for s in (7, 8)])
    w = model.fc1.weight
    out = {"during": probe.seen, "kshard_after": large_of(w).kshard is not None,
           "grad_mode_after": large_of(w).mode}
    torch.distributed.barrier()
    if rank == 0 and not out["kshard_after"] and out["grad_mode_after"] != "ksharded":
        # rank-local inference (a load of the best checkpoint, test, predict on one rank) against a cold twin that has
        # never been sharded: the same kernels on the same weights
        x = _rank_batch(dev, 9)
        twin = Model(**SMALL, precision="bf16").to(dev)
        twin.load_state_dict(model.state_dict())
        with torch.no_grad():
            out["y"], out["y_twin"] = model(x).cpu(), twin(x).cpu()
    return out


def case_nan(rank, world, dev, out_path):
    """terminate_on_nan in ksharded mode: a NaN loss on every rank must raise before fc1's shard, moments or step change."""
    from predict_pv_yield_amd import lightning as pl
    torch.manual_seed(518)
    model = Model(**SMALL, precision="bf16").to(dev)
    out = {}

    class Loader:
        def __len__(self):
            return 2

        def __iter__(self):
            yield _rank_batch(dev, 7)
            ks = large_of(model.fc1.weight).kshard     # (the first step has been queued: the copies below follow it on the stream)
            out["before"] = {k: (ks[k].cpu().clone() if torch.is_tensor(ks[k]) else ks[k])
                             for k in ("w", "shadow", "exp_avg", "exp_avg_sq", "step")}
            yield _rank_batch(dev, 8, nan=True)

    trainer = pl.Trainer(gpus=1, max_epochs=1, large_grad_mode="ksharded", terminate_on_nan=True)
    try:
        trainer.fit(model, Loader())
        out["raised"] = None
    except ValueError as e:
        out["raised"] = str(e)
    torch.cuda.synchronize()
    ks = large_of(model.fc1.weight).kshard
    out["after"] = {k: (ks[k].cpu().clone() if torch.is_tensor(ks[k]) else ks[k])
                    for k in ("w", "shadow", "exp_avg", "exp_avg_sq", "step")}
    out["mode"] = trainer.optimizers[0].large_grad_mode
    return out


BIG = dict(SMALL, history_minutes=55, forecast_minutes=30, image_size_pixels=64)


def case_broadcast(rank, world, dev, out_path):
    """Ranks seeded differently build their operand caches in a no-grad forward, then take rank 0's parameters
    (broadcast_parameters): every rank's next forward must be rank 0's.  fp32 on the 64-pixel model, whose layers take the
    half-float split form (its cached split2 weight images), bf16 on the reduced one (packed conv images, fc1's shadow)."""
    out = {}
    for precision, kw, t in (("bf16", SMALL, 25), ("fp32", BIG, 18)):
        torch.manual_seed(1000 + rank)
        model = Model(**kw, precision=precision).to(dev)
        g = torch.Generator().manual_seed(21)
        x = {"satellite": {"data": torch.randn(4, 11, t, kw["image_size_pixels"], kw["image_size_pixels"], generator=g).to(dev)},
             "pv": {"pv_yield": torch.rand(4, t, 128, generator=g).to(dev)}}
        with torch.no_grad():
            model(x)
        cached = [n for n, p in model.named_parameters()
                  if getattr(p, "_pv_split2" if precision == "fp32" else "_pv_packed", None) is not None]
        D.broadcast_parameters(model)
        with torch.no_grad():
            y = model(x)
        torch.cuda.synchronize()
        out[precision] = {"y": y.cpu(), "cached": cached}
    return out


CASES = {"case_reload": case_reload, "case_after_fit": case_after_fit, "case_nan": case_nan, "case_broadcast": case_broadcast}


def main():
    mode, out_path, steps = sys.argv[1], sys.argv[2], int(sys.argv[3])
    D.init_from_env(force=True)
    assert D.is_distributed()
    rank, world = torch.distributed.get_rank(), torch.distributed.get_world_size()
    dev = torch.device("cuda", D.local_device_index())
    if mode in CASES:
        HipAdam.FUSE_MIN_NUMEL = int(os.environ.get("PV_TEST_FUSE_MIN_NUMEL", "1"))
        os.chdir(os.path.dirname(os.path.abspath(out_path)))       # (a Trainer's files, if any, beside the output)
        out = CASES[mode](rank, world, dev, out_path)
        torch.cuda.synchronize()
        torch.save(out, out_path if rank == 0 else f"{out_path}.rank{rank}")
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
        return
    # the reduced model's fc1 counts as the "large" layer (with 8 ranks only fc1: the other matrices' rows do not divide by 8,
    # and a large layer that cannot be row-sharded moves the whole job to the all-reduce)
    HipAdam.FUSE_MIN_NUMEL = int(os.environ.get("PV_TEST_FUSE_MIN_NUMEL", "1"))
    torch.manual_seed(518)
    model = Model(**SMALL, precision="bf16").to(dev)
    D.broadcast_parameters(model)
    opt = model.configure_optimizers()
    opt.grad_scale = 1.0 / world
    opt.set_large_grad_mode(mode)
    sync = D.OverlappedGradSync(model, large_numel=model.fc1.weight.numel())
    g = torch.Generator().manual_seed(7)
    n_global = int(os.environ.get("PV_TEST_GLOBAL_BATCH", "4"))
    sat = torch.randn(n_global, 11, 25, 16, 16, generator=g)
    pv = torch.rand(n_global, 25, 128, generator=g)
    lo, hi = D.shard_range(n_global)      # each rank trains on its contiguous share of the global batch
    batch = {"satellite": {"data": sat[lo:hi].to(dev)}, "pv": {"pv_yield": pv[lo:hi].to(dev)}}
    losses = []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        loss = model.training_step(batch, 0)
        loss.backward()
        sync.finish()
        opt.step()
        losses.append(float(loss.detach()))
    y = model(batch).detach().cpu()        # forward AFTER the last step: waits for the all-gathered operand copy
    opt.consolidate_sharded()
    torch.cuda.synchronize()
    assert opt.large_grad_mode == mode, (opt.large_grad_mode, mode)
    if rank == 0:
        torch.save({"backend": torch.distributed.get_backend(), "world": world, "state": {k: v.cpu() for k, v in model.state_dict().items()}, "losses": losses, "y": y,
                    "exp_avg_fc1": opt.state[model.fc1.weight]["exp_avg"].cpu(), "mode": opt.large_grad_mode}, out_path)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
