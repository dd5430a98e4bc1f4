"""How tools/time_nbXX.py time a notebook frame predictor, stated once: the train step eagerly and replayed as a HIP graph by
the wall clock, and every conv launch of the step by device events against the same launch on the general Conv3d f32 route
and on torch's own kernels.  Warm-up first, inputs resident before the timed region, INNER back-to-back calls per event pair,
REPS samples of the three routes in turn (ours, general, torch, ours, ...), the median of each with its min and max as the
spread.  A tool passes the warm-up count, INNER and REPS it has always used; they are part of what its recorded figures mean."""
import time
from typing import NamedTuple, Optional

import torch

from predict_pv_yield_amd.graphs import GraphedTrainStep
from predict_pv_yield_amd.optim import HipAdam


def wall(fn, reps, warmup=2):
    """Seconds per call over `reps` calls between two device synchronisations, after `warmup` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def graph_and_eager(model_cls, batch, lr, reps, warmup=2):
    """(the eager model, eager seconds per step, replayed seconds per step): one model stepped eagerly with its own optimizer,
    a second from the same seed captured by GraphedTrainStep and replayed."""
    torch.manual_seed(0)
    model = model_cls().to(batch[next(iter(batch))].device)
    opt = model.configure_optimizers()

    def step():
        opt.zero_grad(set_to_none=True)
        model.training_step(batch, 0).backward()
        opt.step()

    eager = wall(step, reps, warmup)
    torch.manual_seed(0)
    gmodel = model_cls().to(batch[next(iter(batch))].device)
    graphed = GraphedTrainStep(gmodel, HipAdam(gmodel.parameters(), lr=lr, capturable=True), batch, warmup=warmup)
    replay = wall(lambda: graphed(batch), reps, warmup)
    graphed.close()
    return model, eager, replay


def device_ms(fn, inner):
    """Milliseconds per call of `inner` back-to-back calls between two device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def usable(fn, what=None):
    """None where the route takes the launch, else its message (printed after `what`): such a launch is reported, not timed.
    A route that is None is not given: not timed either, and nothing is printed."""
    if fn is None:
        return "not given"
    try:
        fn()
        torch.cuda.synchronize()
        return None
    except Exception as e:
        why = f"{type(e).__name__}: {str(e)[:200]}"
        if what:
            print(f"{what}: {why}")
        return why


class Stat(NamedTuple):
    med: float                  # nan where the route was not timed
    lo: Optional[float]
    hi: Optional[float]

    def __bool__(self):
        return self.lo is not None


def stat(v):
    return Stat(sorted(v)[len(v) // 2], min(v), max(v)) if v else Stat(float("nan"), None, None)


class Row(NamedTuple):
    name: str
    gflop: float
    ours: Stat
    general: Stat               # false where the general route refuses the launch
    torch: Stat
    why_general: Optional[str]  # the refusal's message


def time_cases(cases, reps, inner, warmup, general_name="general route"):
    """One Row per (name, gflop, ours, general, torch) case, yielded as it is measured."""
    for name, gflop, ours, general, torch_fn in cases:
        for _ in range(warmup):
            ours()
        why_g, why_t = usable(general, f"{name}: {general_name}"), usable(torch_fn, f"{name}: torch")
        ta, tg, tt = [], [], []
        for _ in range(reps):     # alternate the three
            ta.append(device_ms(ours, inner))
            if why_g is None:
                tg.append(device_ms(general, inner))
            if why_t is None:
                tt.append(device_ms(torch_fn, inner))
        yield Row(name, gflop, stat(ta), stat(tg), stat(tt), why_g)


def totals():
    return dict.fromkeys(("ours", "general", "torch", "gflop"), 0.0)


def add(tot, row):
    """Adds a row's medians (0 for a route that was not timed) and its GFLOP to the sums of totals()."""
    tot["ours"] += row.ours.med
    tot["general"] += row.general.med if row.general else 0.0
    tot["torch"] += row.torch.med if row.torch else 0.0
    tot["gflop"] += row.gflop


def r4(v):
    return round(v, 4) if v is not None and v == v else None


def spread(s):
    return f"{s.lo:7.3f}-{s.hi:7.3f}" if s else f"{'':15s}"


# ---- the two table forms the tools print, and the JSON record of a row in each ----------------------------------------------
PEAK_TFLOPS = 157.3      # f32 matrix peak of the MI355X at its 2.4 GHz engine clock


def step_line(tag, batch, side, eager, replay, digits=1):
    return (f"{tag} LitAutoEncoder B={batch} {side}x{side}: eager {eager * 1e3:.3f} ms/step ({batch / eager:.{digits}f} samples/s), "
            f"HIP graph {replay * 1e3:.3f} ms/step ({batch / replay:.{digits}f} samples/s)")


def spread_header(width):
    return (f"{'launch':{width}s} {'GFLOP':>7s} {'ours ms':>8s} {'spread':>15s} {'general ms':>10s} {'spread':>15s} {'ours/gen':>8s} "
            f"{'torch ms':>9s}")


def spread_line(r, width):
    ratio = r.ours.med / r.general.med if r.general else float("nan")
    return (f"{r.name:{width}s} {r.gflop:7.3f} {r.ours.med:8.3f} {spread(r.ours)} {r.general.med:10.3f} {spread(r.general)} "
            f"{ratio:8.3f} {r.torch.med:9.3f}")


def spread_total_line(what, width, tot):
    ratio = tot["ours"] / tot["general"] if tot["general"] else float("nan")
    return (f"{what:{width}s} {tot['gflop']:7.3f} {tot['ours']:8.3f} {'':15s} {tot['general']:10.3f} {'':15s} {ratio:8.3f} "
            f"{tot['torch']:9.3f}")


def spread_record(r, **first):
    """A row with its spreads: launch, the tool's own keys, then the times of ours and the general route, and torch's median."""
    return {"launch": r.name, **first, "gflop": round(r.gflop, 4), "ours_ms": r4(r.ours.med), "ours_ms_min": r4(r.ours.lo),
            "ours_ms_max": r4(r.ours.hi), "general_ms": r4(r.general.med), "general_ms_min": r4(r.general.lo),
            "general_ms_max": r4(r.general.hi),
            "ours_over_general": round(r.ours.med / r.general.med, 4) if r.general else None, "torch_ms": r4(r.torch.med)}


def peak_header(width):
    return f"{'launch':{width}s} {'GFLOP':>7s} {'ours ms':>8s} {'of peak':>7s} {'general ms':>10s} {'torch ms':>9s}"


def peak_line(r, width):
    return (f"{r.name:{width}s} {r.gflop:7.2f} {r.ours.med:8.3f} {r.gflop / r.ours.med / PEAK_TFLOPS:7.3f} {r.general.med:10.3f} "
            f"{r.torch.med:9.3f}")


def peak_total_line(width, tot):
    return (f"{'conv launches of a step (median each, summed)':{width}s} {tot['gflop']:7.2f} {tot['ours']:8.3f} "
            f"{tot['gflop'] / tot['ours'] / PEAK_TFLOPS:7.3f} {tot['general']:10.3f} {tot['torch']:9.3f}")


def peak_record(r, **first):
    """A row with its fraction of the f32 matrix peak: launch, the tool's own keys, then gflop, ours, of_peak, general, torch."""
    return {"launch": r.name, **first, "gflop": round(r.gflop, 3), "ours_ms": round(r.ours.med, 4),
            "of_peak": round(r.gflop / r.ours.med / PEAK_TFLOPS, 4), "general_ms": r4(r.general.med), "torch_ms": r4(r.torch.med)}
