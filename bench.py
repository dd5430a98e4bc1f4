#!/usr/bin/env python
"""bench.py — headline benchmark of the MI355X hot path (BASELINE.json metric, configs[1]).

  python bench.py --gpus 1 --steps 20 --warmup 5
  python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs DIR      # + the last step's loss and parameters as .npy
  python bench.py --gpus 1 --full                                         # + every secondary leg below
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
         bench.py --gpus N --steps K --warmup W

A "step" is one train step of the Conv3D PV-yield model (forward + NMAE loss + backward + Adam [+ gradient
exchange over RCCL when N > 1]) on one batch of synthetic PV-site crop stacks [B, 11, 18, 64, 64]
(12 observed + 6 forecast frames) already resident in HBM.  Per-GPU batch is fixed
(weak scaling).  A plain run sets up, warms up, times K steps, writes --dump-outputs if asked, and rank 0 prints ONE JSON
line with the whole-job samples/s and ms_per_step.  With --full the line also carries the in-process device calibration, the
clocks sampled during the timed steps, under N > 1 the other fc1 exchanges (grad_sync_modes) and, at N = 1 (all of it
OUTSIDE the timed region, GPU legs first, the CPU leg last):
  roofline      the single largest kernel of the step (fc1's fused wgrad + Adam pass, HBM-bound) with the Conv3D
                implicit-GEMM family (MFMA-bound) beside it under "mfma_conv3d"; every duration is measured IN THE STEP
                with HIP events around each launch on the launching stream (a few extra, instrumented steps);
  config3       BASELINE configs[2]: joined train step (raw counts -> Farnebäck advection -> Conv3D) and a roofline
                PER STAGE of the advection pipeline (pv_stage_timing: HIP events at every stage boundary);
  fp32          the same headline step on the exact-f32 kernels (precision="fp32");
  val_nmae      "at matched validation NMAE": seeds x 512 Adam steps at B = 32, HIP bf16 against HIP fp32 on the same weights
                and batches, validation NMAE on 1 024 held-out samples averaged over the last 64 steps; gate: |mean paired
                difference| <= 2e-3 AND its standard error <= 7e-4 (seeds added in blocks of 8 until the second holds);
                the torch-CPU oracle follows seed 0 for its time budget (first-steps train losses, two scorers);
  cpu_baseline  those oracle steps, timed, at the benched batch (identical arithmetic to the reference's Lightning path).
"""
import argparse
import contextlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MFMA_BF16_PEAK = 2.5e15     # dense bf16, /opt/skills/guides/MI355X_MICROARCH.md
MFMA_F32_PEAK = 157.3e12    # f32 matrix cores (xf32-free exact f32)
HBM_PEAK = 8.0e12
PROFILE_ROUND = "r06"
TRAFFIC_PROFILE = os.path.join("profiles", PROFILE_ROUND, "pmc_hbm_traffic_bench_B32.json")
FLOW_TRAFFIC_PROFILE = os.path.join("profiles", PROFILE_ROUND, "pmc_flow_traffic_B32.json")
# advection stage -> (kernel of the committed PMC passes, its SQ-counter summary): tools/pmc_flow.sh
FLOW_STAGE_KERNELS = {
    "prepare_stacks (raw -> u8 stacks + normalised frames)": ("pv::prepare_stacks_kernel<short>", "pmc_flow_prepare_stacks.json"),
    "farneback.coarse.prep_polyexp": ("pv::fb_prep_polyexp_mfma_kernel<true>", "pmc_flow_fb_prep_polyexp_mfma_kernel_true_.json"),
    "farneback.level0.prep_polyexp": ("pv::fb_prep_polyexp_mfma_kernel<false>", "pmc_flow_fb_prep_polyexp_mfma_kernel_false_.json"),
    "farneback.level0.iterations_fused": ("pv::fb_level_u_kernel<1, false>", "pmc_flow_fb_level_u_kernel_1__false_.json"),
    "farneback.coarse.iterations_fused": ("pv::fb_level_u_kernel<2, true>", "pmc_flow_fb_level_u_kernel_2__true_.json"),
    "flow_weighted_mean": ("pv::weighted_mean_kernel<4>", "pmc_flow_weighted_mean.json"),
    "remap_bilinear": ("pv::remap_lds_kernel<float>", "pmc_flow_remap_lds.json"),
}

MODEL_KW = dict(include_pv_yield=False, include_nwp=False, forecast_minutes=30, number_of_conv3d_layers=4,
                conv3d_channels=32, image_size_pixels=64, number_sat_channels=11, fc1_output_features=128,
                fc2_output_features=128, fc3_output_features=64, output_variable="pv_yield")


# ------------------------------------------------------------------------------------------------------------------
# in-step kernel timing: HIP events around every launch of the C ABI, on the stream it launches on
# ------------------------------------------------------------------------------------------------------------------
class LaunchTimer:
    """Wraps the functions of predict_pv_yield_amd.hip_ops (functional.py looks them up at call time) so that every call
    is bracketed by two HIP events recorded on torch's current stream == the stream the C ABI launches on."""

    def __init__(self, names):
        from predict_pv_yield_amd import hip_ops as K
        self.K, self.names, self.records, self._saved = K, names, [], {}

    def _key(self, name, args, kwargs):
        t = next((a for a in args if isinstance(a, torch.Tensor)), None)
        shape = tuple(t.shape) if t is not None else ()
        extra = ""
        if name == "conv3d_fwd_bf16":
            pad = kwargs.get("padding", args[6] if len(args) > 6 else (0, 0, 0))
            ncdhw = kwargs.get("y_ncdhw", args[8] if len(args) > 8 else False)
            gated = kwargs.get("out_gate") is not None
            extra = "dgrad" if tuple(pad) == (2, 2, 2) else ("fwd_ncdhw" if ncdhw else "fwd")
            extra += "+gate" if gated else ""
        return name, shape, extra

    def __enter__(self):
        for name in self.names:
            fn = getattr(self.K, name)
            self._saved[name] = fn

            def wrapped(*args, _fn=fn, _name=name, **kwargs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = _fn(*args, **kwargs)
                e1.record()
                self.records.append((self._key(_name, args, kwargs), e0, e1))
                return out

            setattr(self.K, name, wrapped)
        return self

    def __exit__(self, *exc):
        for name, fn in self._saved.items():
            setattr(self.K, name, fn)
        return False

    def summary(self):
        torch.cuda.synchronize()
        acc = {}
        for key, e0, e1 in self.records:
            acc.setdefault(key, []).append(e0.elapsed_time(e1) * 1e-3)
        if os.environ.get("PV_BENCH_DEBUG_BRACKETS"):
            for k, v in acc.items():
                print("[brackets]", k, [round(x * 1e6, 1) for x in v], file=sys.stderr)
        # the MEDIAN over the instrumented steps: a bracket also holds whatever the host does between the first event and the
        # launch (output allocations), which shows when the device has run dry -- the first launch after a synchronisation read
        # 557 us once where its kernel takes 66 (round 6); the mean carried that into the roofline fractions
        import statistics
        return {k: (statistics.median(v), len(v)) for k, v in acc.items()}     # seconds per launch, launches


TIMED_OPS = ("conv3d_fwd_bf16", "conv3d_fwd_bf16_f32in", "conv3d_bwd_weight_bf16", "linear_wgrad_adam_bf16",
             "linear_wgrad_dx_adam_bf16",
             "linear_fwd_bf16", "linear_bwd_bf16", "repack_gate_ncdhw_to_ndhwc_bf16", "adam_step_multi",
             "conv3d_pack_weights_multi")


DUMP_SAMPLE = 1 << 22      # --dump-outputs: a parameter with more elements is written as a fixed, seeded sample (16 MB in f32)


def dump_outputs(out_dir, model, opt, loss, distributed, rank):
    """--dump-outputs: what the timed path hands its caller after its last step -- the loss and every parameter Adam left
    (state_dict(): fc1.weight in the reference's column order) -- as float32 DIR/<name>.npy.  A parameter of more than
    DUMP_SAMPLE elements (fc1.weight, 128 M) is written as DIR/<name>.sample.npy: the values at DUMP_SAMPLE flat indices drawn
    once from a generator seeded with 518, in ascending order.  Under N > 1 the sharded parameters are gathered first
    (collective) and rank 0 writes."""
    import numpy as np
    if distributed:
        opt.consolidate_sharded()
    if rank != 0:
        return
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "loss.npy"), loss.detach().float().reshape(1).cpu().numpy())
    for name, t in model.state_dict().items():
        t = t.detach().float()
        if t.numel() > DUMP_SAMPLE:
            idx = torch.randint(0, t.numel(), (DUMP_SAMPLE,), generator=torch.Generator().manual_seed(518)).sort().values
            np.save(os.path.join(out_dir, name + ".sample.npy"), t.reshape(-1)[idx.to(t.device)].cpu().numpy())
        else:
            np.save(os.path.join(out_dir, name + ".npy"), t.cpu().numpy())


def settle():
    """Between two legs: collect what the last one left (models and optimisers sit in reference cycles -- a parameter's
    fused-backward closure holds its optimiser -- so `del` alone frees nothing), then hand the cached blocks back.  Otherwise the
    collector runs whenever it pleases INSIDE the next leg's timed loop: freeing a captured graph's 3.6 GB there cost the T = 19
    sweep one 87 ms stall (5.2 ms per step over 30 steps instead of 1.8: tools/probes/t19_after_graph.py)."""
    import gc
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def committed_hbm_traffic():
    """HBM bytes per launch from the COMMITTED PMC passes (tools/pmc_traffic.py: separate --pmc FETCH_SIZE / WRITE_SIZE runs
    of this bench, gfx950-corrected).  PMC counters cannot be collected from inside the timed run."""
    path = os.path.join(ROOT, TRAFFIC_PROFILE)
    if not os.path.exists(path):
        return {}
    return json.load(open(path))["kernels"]


def committed_flow_traffic(b):
    """HBM bytes of one batch of the advection pipeline from the committed FETCH_SIZE / WRITE_SIZE passes over
    tools/time_flow_stages.py (tools/pmc_flow_traffic.py; {} until a collection for this batch size is committed)."""
    path = os.path.join(ROOT, FLOW_TRAFFIC_PROFILE)
    if not os.path.exists(path):
        return {}
    d = json.load(open(path))
    return d if d.get("batch") == b else {}


def measure_step_rooflines(step, model, b, t_frames, n_steps=5):
    """Runs n instrumented steps (same tensors, same launch sequence as the timed region) and prices the kernels."""
    with LaunchTimer(TIMED_OPS) as lt:
        step()                      # one step to get the host ahead of the device again (the timed region ended with a sync)
        lt.records.clear()
        for _ in range(n_steps):
            step()
    per = lt.summary()
    traffic = committed_hbm_traffic()
    kernels, fam_s, fam_fl, fam_n = {}, 0.0, 0.0, 0
    for (name, shape, extra), (secs, n) in sorted(per.items(), key=lambda kv: -kv[1][0] * kv[1][1]):
        per_step = n // n_steps
        entry = {"us_per_launch": round(secs * 1e6, 1), "launches_per_step": per_step}
        if name in ("conv3d_fwd_bf16", "conv3d_bwd_weight_bf16", "conv3d_fwd_bf16_f32in"):
            if name == "conv3d_fwd_bf16_f32in":
                bb, c_in, t, h, w = shape
                vox = (t - 2) * (h - 2) * (w - 2)
            else:
                bb, t, h, w, cpad = shape
                c_in = 11 if cpad == 16 else 32
                vox = t * h * w if extra.startswith("dgrad") else (t - 2) * (h - 2) * (w - 2)
            fl = 2.0 * bb * 32 * c_in * 27 * vox
            entry.update(algorithmic_gflop=round(fl / 1e9, 2), tflops=round(fl / secs / 1e12, 1),
                         frac_of_bf16_mfma_peak=round(fl / secs / MFMA_BF16_PEAK, 4))
            if name == "conv3d_fwd_bf16" and shape[-1] == 32:
                fam_s += secs * per_step
                fam_fl += fl * per_step
                fam_n += per_step
        label = f"{name}[{extra}]{list(shape)}" if extra else f"{name}{list(shape)}"
        kernels[label] = entry
    out = {}
    # --- the single largest kernel of the step: fc1 fused wgrad + Adam (one pass over p, m, v + the bf16 operand copy)
    fc1 = [(k, v) for k, v in per.items() if k[0] in ("linear_wgrad_adam_bf16", "linear_wgrad_dx_adam_bf16")]
    if fc1:
        (name, shape, _), (secs, n) = fc1[0]
        nrows, kcols = model.fc1.weight.shape
        single_pass = name == "linear_wgrad_dx_adam_bf16"
        # p, m, v read + written, shadow written, x read once (+ dx written by the single-pass form)
        byt = nrows * kcols * (3 * 4 * 2 + 2) + b * kcols * 2 * (2 if single_pass else 1)
        kname = "pv::linear_bwd_dw_dx_adam_kernel" if single_pass else "pv::linear_bwd_dw_bf16_kernel<1>"
        # (the one-pass kernel is a template since round 5: "pv::linear_bwd_dw_dx_adam_kernel<2, true>")
        tr = next((v.get("hbm_bytes_per_launch") for k_, v in traffic.items() if k_ == kname or k_.startswith(kname + "<")), None)
        out.update({"bound": "hbm", "kernel": (kname[4:] + " (fc1 backward in one pass: wgrad + Adam + dx + db, 128.45 M weights)")
                    if single_pass else "linear_bwd_dw_bf16_kernel<1> (fc1 wgrad + Adam fused, 128.45 M weights)",
                    "achieved": round(byt / secs / 1e9, 1), "peak": HBM_PEAK / 1e9, "unit": "GB/s",
                    "frac": round(byt / secs / HBM_PEAK, 4), "traffic": tr, "avg_launch_ms": round(secs * 1e3, 4),
                    "launches_per_step": 1, "algorithmic_bytes_per_launch": byt,
                    "share_of_step": None})
    if fam_n:
        fam_tr = [v for k, v in traffic.items() if k.startswith("pv::conv3d_fwd_bf16_v3_kernel")]
        n_tr = sum(v["launches"] for v in fam_tr)
        out["mfma_conv3d"] = {
            "bound": "mfma", "kernel": "conv3d_fwd_bf16_v3_kernel family (32 -> 32 channels: 3 forward + 3 dgrad launches per step)",
            "achieved": round(fam_fl / fam_s / 1e12, 2), "peak": MFMA_BF16_PEAK / 1e12, "unit": "TFLOP/s",
            "frac": round(fam_fl / fam_s / MFMA_BF16_PEAK, 4),
            "traffic": round(sum(v["hbm_bytes_per_launch"] * v["launches"] for v in fam_tr) / n_tr) if n_tr else None,
            "avg_launch_ms": round(fam_s / fam_n * 1e3, 4), "launches_per_step": fam_n,
            "algorithmic_gflop_per_step": round(fam_fl / 1e9, 2)}
    conv_all = [(k, v) for k, v in kernels.items() if "algorithmic_gflop" in v]
    tot_fl = sum(v["algorithmic_gflop"] * v["launches_per_step"] for _, v in conv_all)
    tot_s = sum(v["us_per_launch"] * v["launches_per_step"] for _, v in conv_all)
    out["all_conv_kernels"] = {"gflop_per_step": round(tot_fl, 1), "us_per_step": round(tot_s, 1),
                               "frac_of_bf16_mfma_peak": round(tot_fl * 1e9 / (tot_s * 1e-6) / MFMA_BF16_PEAK, 4)}
    out["all_conv_frac"] = out["all_conv_kernels"]["frac_of_bf16_mfma_peak"]
    # the same launches against the OTHER roof: at 32 channels a conv layer moves 128-192 bytes per 55 kflop, i.e. 290-430 flop / B
    # where the device's ridge is 2.5 PF / 8 TB/s = 312 (470 against the copy rate it reaches): the family draws most of the
    # memory system while it multiplies (PMC bytes of the committed counter passes, per step)
    conv_tr = {k: v for k, v in traffic.items() if k.startswith("pv::conv3d_")}
    n_tr_steps = next((v["launches"] for k, v in conv_tr.items() if k.startswith("pv::conv3d_first_f32in_kernel")), 0)
    if n_tr_steps and tot_s > 0:
        conv_bytes = sum(v["hbm_bytes_per_launch"] * v["launches"] for v in conv_tr.values()) / n_tr_steps
        out["all_conv_kernels"].update({"hbm_GB_per_step": round(conv_bytes / 1e9, 4),
                                        "hbm_TBps": round(conv_bytes / (tot_s * 1e-6) / 1e12, 3),
                                        "frac_of_hbm_peak": round(conv_bytes / (tot_s * 1e-6) / HBM_PEAK, 4)})
        out["all_conv_hbm_frac"] = out["all_conv_kernels"]["frac_of_hbm_peak"]
    if fam_n:
        out["conv_fwd_dgrad_frac"] = out["mfma_conv3d"]["frac"]
    out["kernels"] = kernels
    out["method"] = (f"{n_steps} extra train steps (after one discarded) with a HIP event pair around every launch (torch's current "
                     "stream = the launching stream), median per launch; traffic = committed rocprofv3 --pmc passes (" + TRAFFIC_PROFILE + ")")
    return out


# ------------------------------------------------------------------------------------------------------------------
# config 3: advection pipeline per stage + joined train step
# ------------------------------------------------------------------------------------------------------------------
def measure_config3(dev, b, history_minutes):
    from predict_pv_yield_amd import hip_ops as K
    from predict_pv_yield_amd import optical_flow as of
    from predict_pv_yield_amd.models.conv3d.model import Model
    from predict_pv_yield_amd.data.synthetic import advected_counts
    t_obs, c, hw, n_future = 12, 11, 64, 6
    # the SURVEY section-8(d) workload: dense blob textures advected by a constant sub-pixel velocity, seed 1234 -- the very
    # tensor the CPU leg (flow_cpu_baseline) and tests/test_gpu_headline.py's joined-model parity test use.  The fused
    # iteration's LDS gathers follow the flow, so its time depends on the data: noise is not this workload.
    raw = torch.from_numpy(advected_counts(batch=b, t=t_obs, channels=c, h=hw, w=hw, seed=1234)[0]).to(dev)
    for _ in range(5):
        of.advect_future_frames(raw, n_future)
    iters = 10
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    # the pipeline as the product runs it: back-to-back launches, no events inside; 30 batches, so that the host's head
    # start over an idle device (the first batch's ~25 launches are enqueued while the device waits) is amortised, as in the
    # 100-step timing of the train step
    plain_iters = 30
    e0.record()
    for _ in range(plain_iters):
        of.advect_future_frames(raw, n_future)
    e1.record()
    torch.cuda.synchronize()
    total = e0.elapsed_time(e1) * 1e-3 / plain_iters
    # and once more with a HIP event at every stage boundary (pv_stage_timing) for the per-stage table: the 8 extra event
    # packets per batch cost ~0.2 ms in total (measured: 1.37 ms plain, 1.59 ms staged on the same box), so the stage times
    # add up to more than pipeline_ms
    with K.stage_timing() as st:
        e0.record()
        for _ in range(iters):
            of.advect_future_frames(raw, n_future)
        e1.record()
    torch.cuda.synchronize()
    total_staged = e0.elapsed_time(e1) * 1e-3 / iters
    pairs = b * c * (t_obs - 1)
    px0, px1 = hw * hw, (hw // 2) * (hw // 2)
    # algorithmic work per stage: bytes = compulsory traffic of the stage's inputs/outputs as the stage is
    # defined (R = 5 coefficient channels f32, M = 5 channels f32, flow 2 channels f32), flops per level-pixel:
    # PolyExp 140 per image pixel, UpdateMatrices 75, window blur + solve 620.  The per-image stages run once per FRAME
    # (a frame is `next` of one pair and `prev` of the following one): frames = B * C * T, not 2 * pairs; a level's starting
    # flow is formed inside its first UpdateMatrices (launch group 1 of 3 reads the coarser flow instead of a flow field).
    frames = b * c * t_obs
    alg = {
        "prepare_stacks (raw -> u8 stacks + normalised frames)": dict(bytes=b * t_obs * c * px0 * (2 + 1 + 4), flops=0),
        "farneback.coarse.prep_polyexp": dict(bytes=frames * (px0 + px1 * 20), flops=frames * px1 * 140),
        "farneback.level0.prep_polyexp": dict(bytes=frames * (px0 + px0 * 20), flops=frames * px0 * 140),
        "farneback.coarse.update_matrices": dict(bytes=pairs * px1 * (40 + 8 + 20), flops=pairs * px1 * 75),
        "farneback.level0.update_matrices": dict(bytes=pairs * px0 * (40 + 8 + 20), flops=pairs * px0 * 75),
        "farneback.coarse.window_blur_solve": dict(bytes=pairs * px1 * (20 + 8), flops=pairs * px1 * 620),
        "farneback.level0.window_blur_solve": dict(bytes=pairs * px0 * (20 + 8), flops=pairs * px0 * 620),
        # ONE launch per level runs its three iterations (UpdateMatrices + window blur + solve each) with R0 in registers, R1 and
        # the flow between iterations in LDS: what the launch must move is R0 + R1 once, the starting flow in and the flow out
        # (56 B per pixel and pair); the arithmetic is SURVEY's 3 x (75 + 620) flop per pixel and pair.  (Rounds 3-4 priced this
        # stage at three round trips of those bytes -- the one-launch-per-iteration form -- and read "bound hbm, frac 0.65" off
        # a kernel that moves a third of that and is bound by its vector and matrix instructions: VERDICT r4 weak point 7.)
        "farneback.level0.iterations_fused": dict(bytes=pairs * px0 * (40 + 8 + 8), flops=3 * pairs * px0 * (75 + 620)),
        "farneback.coarse.iterations_fused": dict(bytes=pairs * px1 * (40 + 8 + 8), flops=3 * pairs * px1 * (75 + 620)),
        "flow_weighted_mean": dict(bytes=b * c * px0 * 8 * (t_obs - 1 + 1), flops=b * c * px0 * 2 * 2 * (t_obs - 1)),
        "remap_bilinear": dict(bytes=b * c * n_future * px0 * 16, flops=b * c * n_future * px0 * 10),
    }
    stages = {}
    flow_traffic = committed_flow_traffic(b)
    for label, (ms, count) in st.stages.items():
        secs = ms * 1e-3 / iters
        a = alg.get(label, dict(bytes=0, flops=0))
        per = max(count // iters, 1)
        t_mem, t_fl = a["bytes"] * per / HBM_PEAK, a["flops"] * per / MFMA_F32_PEAK
        bound = "hbm" if t_mem >= t_fl else "compute"
        entry = {"ms": round(secs * 1e3, 4), "launch_groups": per, "bound": bound,
                 "algorithmic_GB": round(a["bytes"] * per / 1e9, 4), "algorithmic_GFLOP": round(a["flops"] * per / 1e9, 2),
                 "GBps": round(a["bytes"] * per / secs / 1e9, 1), "TFLOPs_f32": round(a["flops"] * per / secs / 1e12, 2)}
        # measured HBM bytes of the stage's kernel (committed FETCH_SIZE / WRITE_SIZE passes) next to the algorithmic ones
        kern, sq_file = FLOW_STAGE_KERNELS.get(label, (None, None))
        tk = flow_traffic.get("kernels", {}).get(kern) if kern else None
        if tk and a["bytes"]:
            entry["pmc_GB"] = round(tk["hbm_GB_per_batch"], 4)
            entry["pmc_over_algorithmic"] = round(tk["hbm_GB_per_batch"] * 1e9 / (a["bytes"] * per), 2)
        if bound == "hbm":
            entry["frac"] = round(t_mem / secs, 4)          # of 8 TB/s, on the ALGORITHMIC bytes
            if "prep_polyexp" in label:
                # priced by SURVEY's bytes and flops the stage is memory-side; the IMPLEMENTATION is a latency chain of phases
                # (in-kernel stamps and three negative experiments, profiles/r05/NOTES.md)
                entry["implementation_bound"] = ("latency: per image four phases behind barriers (source, filters, products, epilogue) at two "
                                                 "waves per SIMD; the product phase is a chain LDS read -> product -> re-split -> product "
                                                 "(a quarter fewer matrix instructions changed nothing); not store-bound: write-only kernels "
                                                 "reach 5.4-5.7 TB/s in the same store shape (tools/probes/store_rate.hip, profiles/r05/NOTES.md)")
        else:
            # a stage bound by its instructions: the fraction of the f32 flop peak its SURVEY flops reach, and -- from the
            # committed SQ-counter passes -- how busy the vector and the matrix pipes were while its waves were resident
            entry["frac_of_f32_peak_on_survey_flops"] = round(t_fl / secs, 4)
            sq_path = os.path.join(ROOT, "profiles", PROFILE_ROUND, sq_file) if sq_file else None
            if sq_path and os.path.exists(sq_path):
                cnt = json.load(open(sq_path))
                c_, d_ = cnt.get("counters_per_dispatch", {}), cnt.get("derived", {})
                if c_.get("SQ_WAVE_CYCLES"):
                    entry["valu_issue_over_wave_cycles"] = round(c_.get("SQ_ACTIVE_INST_VALU", 0.0) / c_["SQ_WAVE_CYCLES"], 4)
                entry["matrix_pipe_busy_while_resident"] = d_.get("matrix_pipe_busy_while_resident")
                entry["wait_any_over_wave_cycles"] = d_.get("wait_any_over_wave_cycles")
        stages[label] = entry
    compulsory = b * (t_obs * c * px0 * 2 + n_future * c * px0 * 4)
    # per sample 2.16 MB compulsory (raw counts in, six f32 frames out) and 1.49 GFLOP f32 (121 pairs
    # x 4096 px x 3.0 kflop); the pipeline's roofline is whichever of the two takes longer at its peak
    survey_s = max(compulsory / HBM_PEAK, pairs * px0 * 3.0e3 / MFMA_F32_PEAK)
    out = {"workload": f"raw [B={b},12,11,64,64] int16 -> u8 -> 121 Farneback pairs/sample -> weighted mean -> normalise -> "
                       "6 advected frames written into the model input [B,11,18,64,64]",
           "pipeline_ms": round(total * 1e3, 3), "pipeline_ms_with_stage_events": round(total_staged * 1e3, 3),
           "samples_per_s": round(b / total, 1),
           "farneback_pairs_per_s": round(pairs / total, 0),
           "compulsory_GB": round(compulsory / 1e9, 4), "compulsory_GBps": round(compulsory / total / 1e9, 1),
           "survey_roofline_us": round(survey_s * 1e6, 1), "frac_of_survey_roofline": round(survey_s / total, 4),
           "hbm_traffic_GB": flow_traffic.get("GB_per_batch"),
           "traffic_over_compulsory": round(flow_traffic["GB_per_batch"] * 1e9 / compulsory, 2) if flow_traffic else None,
           "traffic_profile": FLOW_TRAFFIC_PROFILE if flow_traffic else None,
           "input": "data.synthetic.advected_counts(seed=1234): blob textures advected by U(-3,3) px/frame",
           "stages": stages,
           "stage_method": "pv_stage_timing_begin/_end: one HIP event per stage boundary on the launching stream; a stage is "
                           "'hbm'-bound when its algorithmic bytes at 8 TB/s take longer than its SURVEY flops at 157.3 TFLOP/s (then "
                           "frac = algorithmic GB/s / 8 TB/s, and pmc_over_algorithmic says how much more it really moved), else "
                           "'compute'-bound (vector / matrix pipe occupancy from the committed SQ counters instead of a byte fraction)"}
    # joined train step: Model(future_frames="optical_flow") on the raw-count batch
    torch.manual_seed(518)
    model = Model(**MODEL_KW, history_minutes=history_minutes, precision="bf16", future_frames="optical_flow").to(dev)
    model.batch_size = max(model.batch_size, b)
    opt = model.configure_optimizers()
    batch = {"satellite": {"data": raw}, "pv": {"pv_yield": torch.rand(b, 18, 128, device=dev)}}

    def step():
        opt.zero_grad(set_to_none=True)
        model.training_step(batch, 0).backward()
        opt.step()

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 40      # as many as amortise the host's head start over an idle device (the 100-step timing of the headline does)
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    d = (time.perf_counter() - t0) / n
    out["joined_train_step"] = {"ms_per_step": round(d * 1e3, 3), "samples_per_s": round(b / d, 1),
                                "workload": "advection pipeline + conv3d train step (fwd + NMAE + bwd + Adam) per batch"}
    del model, opt
    return out


def measure_engine_clocks(dev, b=32):
    """The engine clock the device really holds under the step's kernel families (hip_ops.engine_clock_under: a one-wave watcher of
    the shader-cycle counter against the 100 MHz counter).  The spec peak (2.5 PFLOP/s) is a 2.4 GHz figure; under the conv kernels'
    matrix + LDS + HBM load the power management holds ~1.7-1.8 GHz, under the bare matrix-instruction loop ~2.15, under a copy 2.4."""
    from predict_pv_yield_amd import hip_ops as K
    from predict_pv_yield_amd._lib import check, current_stream_ptr, get_lib, ptr
    g = torch.Generator(device=dev).manual_seed(1)
    lib = get_lib()
    out = {"what": "median engine clock (MHz) while one kind of kernel loops for 20 ms; idle device and plain copy: 2 400"}
    sink = torch.zeros(4096, device=dev)
    out["bare_mfma_loop"] = K.engine_clock_under(lambda: check(lib.pv_calibrate_mfma_bf16(ptr(sink), 512, 2000, current_stream_ptr())))
    w = torch.randn(32, 32, 3, 3, 3, device=dev, generator=g) * 0.05
    x = torch.randn(b, 16, 62, 62, 32, device=dev, generator=g).relu().to(torch.bfloat16)
    dy = torch.randn(b, 14, 60, 60, 32, device=dev, generator=g).to(torch.bfloat16)
    wp = K.conv3d_pack_weight_bf16(w, transpose_flip=False)
    bias = torch.zeros(32, device=dev)
    out["conv_forward_32_to_32"] = K.engine_clock_under(lambda: K.conv3d_fwd_bf16(x, None, wp, bias, 32, 32, (0, 0, 0), True, False))
    out["conv_weight_gradient"] = K.engine_clock_under(lambda: K.conv3d_bwd_weight_bf16(x, dy, None, 32, 32, (0, 0, 0)))
    del x, dy
    k = 1003520
    xf = torch.randn(b, k, device=dev, generator=g).relu().to(torch.bfloat16)
    wf = torch.randn(128, k, device=dev, generator=g) * 0.01
    m1, v1 = torch.zeros_like(wf), torch.zeros_like(wf)
    sh = K.cast_f32_to_bf16(wf)
    gy, yy = torch.randn(b, 128, device=dev, generator=g) * 1e-3, torch.rand(b, 128, device=dev, generator=g)
    st = [0]

    def fc1():
        st[0] += 1
        K.linear_wgrad_dx_adam_bf16(xf, gy, yy, wf, m1, v1, sh, st[0], need_dx=True, need_db=False, gate_dx_by_x=True)
    out["fc1_one_pass_backward"] = K.engine_clock_under(fc1)
    return out


def measure_graph_step(dev, b, history_minutes, steps=20):
    """The same train step captured ONCE as a HIP graph (graphs.GraphedTrainStep: forward + NMAE + backward + HipAdam with
    its step counter and bias corrections in device memory) and replayed: what is left when no Python, autograd or launch
    work sits between the kernels.  `replay_ms` replays on the resident batch (the headline's condition);
    `with_batch_copy_ms` copies a fresh batch into the graph's static input first."""
    from predict_pv_yield_amd.graphs import GraphedTrainStep
    from predict_pv_yield_amd.models.conv3d.model import Model
    from predict_pv_yield_amd.optim import HipAdam
    torch.manual_seed(518)
    model = Model(**MODEL_KW, history_minutes=history_minutes, precision="bf16").to(dev)
    model.batch_size = max(model.batch_size, b)
    t = model.history_len_5 + model.forecast_len_5 + 1
    g = torch.Generator(device=dev).manual_seed(518)
    batch = {"satellite": {"data": torch.randn(b, 11, t, 64, 64, generator=g, device=dev)},
             "pv": {"pv_yield": torch.rand(b, t, 128, generator=g, device=dev)}}
    opt = HipAdam(model.parameters(), lr=5e-4, capturable=True)
    step = GraphedTrainStep(model, opt, batch, warmup=3)
    for _ in range(3):
        step.graph.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step.graph.replay()
    torch.cuda.synchronize()
    d = (time.perf_counter() - t0) / steps
    t0 = time.perf_counter()
    for _ in range(steps):
        step(batch)
    torch.cuda.synchronize()
    d2 = (time.perf_counter() - t0) / steps
    out = {"replay_ms": round(d * 1e3, 3), "samples_per_s": round(b / d, 1), "with_batch_copy_ms": round(d2 * 1e3, 3),
           "loss_after": round(float(step.static_loss), 6), "optimizer_steps_on_device": opt.device_step(),
           "what": "forward + NMAE + backward + Adam of the headline step as ONE captured HIP graph, replayed"}
    step.close()      # release the graph, its pinned workspaces and the optimiser's frozen layout NOW, not at some later collection
    del step, model, opt
    return out


def measure_batch_sweep(dev, history_minutes, batches=(8, 64), steps=10, warmup=3):
    """The same bf16 train step at the other per-GPU batch sizes of SURVEY.md §8d: the fc1 update (0.6 ms) is a fixed cost
    per step, so samples/s grows with the batch."""
    from predict_pv_yield_amd.models.conv3d.model import Model
    out = {}
    for b in batches:
        torch.manual_seed(518)
        model = Model(**MODEL_KW, history_minutes=history_minutes, precision="bf16").to(dev)
        model.batch_size = max(model.batch_size, b)
        opt = model.configure_optimizers()
        t = model.history_len_5 + model.forecast_len_5 + 1
        g = torch.Generator(device=dev).manual_seed(518)
        batch = {"satellite": {"data": torch.randn(b, 11, t, 64, 64, generator=g, device=dev)},
                 "pv": {"pv_yield": torch.rand(b, t, 128, generator=g, device=dev)}}

        def step():
            opt.zero_grad(set_to_none=True)
            model.training_step(batch, 0).backward()
            opt.step()

        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        d = (time.perf_counter() - t0) / steps
        out[f"B={b}"] = {"ms_per_step": round(d * 1e3, 3), "samples_per_s": round(b / d, 1)}
        del model, opt, batch
        settle()
    return out


def measure_sharded_rank_compute(dev, history_minutes, world=8, global_batch=512, steps=10, warmup=3):
    """What ONE rank of the strong-scaling run computes per step, measured on this one GPU without any exchange: per-GPU batch
    global_batch / world, fc1's gradient written once as bf16 (pv_linear_wgrad_bf16out), Adam over this rank's 1 / world of the
    rows (the row shard of HipAdam's "sharded" mode), the other kernels as in every mode.  The reduce-scatter and the
    all-gather are left out (their inputs / outputs exist, nothing moves): world x (global_batch / world) / this time is the
    aggregate rate the job reaches if the exchange hides completely -- the ceiling the measured 8-GPU number is read against
    (it decides whether 6 x over the one-GPU global-batch run is reachable at all)."""
    from unittest import mock
    from predict_pv_yield_amd import distributed as D
    from predict_pv_yield_amd.models.conv3d.model import Model
    b = global_batch // world
    torch.manual_seed(518)
    model = Model(**MODEL_KW, history_minutes=history_minutes, precision="bf16").to(dev)
    model.batch_size = max(model.batch_size, b)
    opt = model.configure_optimizers()
    opt.grad_scale = 1.0 / world
    rows = model.fc1.weight.shape[0]
    if rows % world:
        return {"skipped": f"fc1's {rows} rows do not divide over {world} ranks"}
    shard = (0, rows // world)
    t = model.history_len_5 + model.forecast_len_5 + 1
    g = torch.Generator(device=dev).manual_seed(518)
    batch = {"satellite": {"data": torch.randn(b, 11, t, 64, 64, generator=g, device=dev)},
             "pv": {"pv_yield": torch.rand(b, t, 128, generator=g, device=dev)}}
    with mock.patch.object(D, "row_shard", lambda n_rows, rank=None, world=None: shard), \
            mock.patch.object(D, "all_gather_rows", lambda full, async_op=True: None):
        opt.set_large_grad_mode("sharded")
        for p in opt.large_params():        # the hand-over OverlappedGradSync installs, minus the reduce-scatter itself
            p._pv_on_grad = lambda gb, param=None: setattr(param, "_pv_grad_shard", gb[shard[0]:shard[1]])

        def step():
            opt.zero_grad(set_to_none=True)
            model.training_step(batch, 0).backward()
            opt.step()

        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        d = (time.perf_counter() - t0) / steps
    mode = opt.large_grad_mode
    del model, opt, batch
    settle()
    return {"ms_per_step": round(d * 1e3, 3), "per_gpu_batch": b, "emulated_world": world, "rows_stepped": shard[1], "mode": mode,
            "aggregate_samples_per_s_if_exchange_hides": round(world * b / d, 1),
            "exchange_bytes_per_rank_and_step": {"reduce_scatter_in_bf16": rows * model_k(t) * 2,
                                                 "all_gather_out_bf16": rows * model_k(t) * 2},
            "what": "one rank's kernels of bench.py --gpus 8 --global-batch 512 (sharded fc1 update), no exchange"}


def measure_ksharded_rank_compute(dev, history_minutes, world=8, per_gpu_batch=64, steps=10, warmup=3):
    """One rank's kernels of the K-SHARDED run (HipAdam large_grad_mode "ksharded") on this one GPU, no exchange: the conv tower
    on per_gpu_batch samples, the staging copies of the two all-to-alls, fc1's forward / input gradient / weight gradient + Adam
    on this rank's 1 / world of the COLUMNS for world x per_gpu_batch rows.  The collectives are replaced by local stand-ins of
    the same shapes (the send-side staging copy of an all-to-all is kept, the wire is not)."""
    from unittest import mock
    from predict_pv_yield_amd import distributed as D
    from predict_pv_yield_amd import hip_ops as K
    from predict_pv_yield_amd.models.conv3d.model import Model
    b = per_gpu_batch
    torch.manual_seed(518)
    model = Model(**MODEL_KW, history_minutes=history_minutes, precision="bf16").to(dev)
    model.batch_size = max(model.batch_size, b)
    opt = model.configure_optimizers()
    opt.grad_scale = 1.0 / world
    n, k = model.fc1.weight.shape
    if k % (world * K.MOMENT_TILE):
        return {"skipped": f"fc1's {k} columns do not divide over {world} ranks in multiples of {K.MOMENT_TILE}"}
    kr = k // world
    t = model.history_len_5 + model.forecast_len_5 + 1
    g = torch.Generator(device=dev).manual_seed(518)
    batch = {"satellite": {"data": torch.randn(b, 11, t, 64, 64, generator=g, device=dev)},
             "pv": {"pv_yield": torch.rand(b, t, 128, generator=g, device=dev)}}
    # (the staging copies of the two all-to-alls as distributed.py makes them, without the exchange between them)
    fwd = lambda x: D._swap01(x.contiguous().view(x.shape[0], world, kr)).view(world * x.shape[0], kr)
    back = lambda d: D._swap01(d.contiguous().view(world, d.shape[0] // world, kr)).view(d.shape[0] // world, world * kr)
    ww = world
    with mock.patch.object(D, "is_distributed", lambda: True), \
            mock.patch.object(D, "column_shard", lambda n_cols, rank=None, world=None, multiple=8: (0, n_cols // ww)), \
            mock.patch.object(D, "all_to_all_columns", fwd), mock.patch.object(D, "all_to_all_rows_back", back), \
            mock.patch.object(D, "reduce_scatter_sample_rows",
                              lambda p: K.colsum(p.view(world, p.numel() // world)).view(p.shape[0] // world, p.shape[1])), \
            mock.patch.object(D, "all_gather_sample_rows", lambda loc: loc.repeat(world, 1)):
        opt.set_large_grad_mode("ksharded")
        if opt.large_grad_mode != "ksharded":
            return {"skipped": f"the optimiser chose '{opt.large_grad_mode}'"}

        def step():
            opt.zero_grad(set_to_none=True)
            model.training_step(batch, 0).backward()
            opt.step()

        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        d = (time.perf_counter() - t0) / steps
        for p in opt.large_params():
            p._pv_kshard = None
        opt.large_grad_mode = "autograd"
    ex = exchange_bytes("ksharded", world, b, model)
    del model, opt, batch
    settle()
    return {"ms_per_step": round(d * 1e3, 3), "per_gpu_batch": b, "emulated_world": world, "columns_stepped": kr, "mode": "ksharded",
            "aggregate_samples_per_s_if_exchange_hides": round(world * b / d, 1), "exchange_bytes_per_rank_and_step": ex,
            "what": "one rank's kernels of bench.py --gpus 8 --grad-sync ksharded (fc1's columns dealt over the ranks), no exchange"}


def model_k(t_frames):
    return 32 * (t_frames - 8) * 56 * 56      # fc1 input features of the headline model


def measure_fp32_headline(dev, b, history_minutes, steps=5):
    from predict_pv_yield_amd.models.conv3d.model import Model
    torch.manual_seed(518)
    model = Model(**MODEL_KW, history_minutes=history_minutes, precision="fp32").to(dev)
    model.batch_size = max(model.batch_size, b)
    opt = model.configure_optimizers()
    t = model.history_len_5 + model.forecast_len_5 + 1
    g = torch.Generator(device=dev).manual_seed(518)
    batch = {"satellite": {"data": torch.randn(b, 11, t, 64, 64, generator=g, device=dev)},
             "pv": {"pv_yield": torch.rand(b, t, 128, generator=g, device=dev)}}

    def step():
        opt.zero_grad(set_to_none=True)
        model.training_step(batch, 0).backward()
        opt.step()

    for _ in range(2):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    d = (time.perf_counter() - t0) / steps
    return {"dtype": "fp32", "ms_per_step": round(d * 1e3, 3), "value": round(b / d, 1), "unit": "samples/s",
            "steps": steps, "per_gpu_batch": b,
            # the step's 23.37 GFLOP per sample over the f32 matrix peak: an EQUIVALENT rate (it can exceed 1) -- since round 5 only
            # fc1's forward and dx (0.52 GFLOP per sample) issue on the f32 pipe; every conv product runs as three half-float
            # products on the 16-bit matrix cores
            "equivalent_f32_flops_over_f32_peak": round(b / d * 23.37e9 / MFMA_F32_PEAK, 4),
            "f32_pipe_share_of_flops": round(0.52 / 23.37, 3),
            "note": "precision=\"fp32\": conv forward / data gradient / weight gradient as two-term half-float splits (three matrix-core products each, f32 accumulation, 4e-6 of float64), fc1 forward and dx with exact f32 products (v_mfma_f32_32x32x2f32), its weight gradient inside the f32 Adam pass; rtol 1e-4 parity path, same step definition"}


def measure_other_models(dev):
    """Train-step throughput of the other models built on the same kernels (not the headline metric; outside the timed
    region): the optical-flow notebook's 3-D CNN at its own batch size, and the PerceiverModel at the reference's
    configs/model/perceiver.yaml (T = 19, 64 x 64, batch 8)."""
    out = {}

    def time_steps(step, n, warm):
        for _ in range(warm):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    from predict_pv_yield_amd.models.conv3d import flow_autoencoder as fa
    torch.manual_seed(0)
    g = torch.Generator(device=dev).manual_seed(1)
    b = 64
    batch = {fa.HISTORICAL_SAT_IMAGES: torch.randn(b, 4, 128, 128, generator=g, device=dev),
             fa.OPTICAL_FLOW_PREDICTIONS: torch.randn(b, 128, 128, generator=g, device=dev),
             fa.FORECAST_HORIZON: torch.randn(b, generator=g, device=dev),
             fa.TARGET_SAT_IMAGE: torch.randn(b, 64, 64, generator=g, device=dev)}
    ae = fa.LitAutoEncoder().to(dev)
    opt = ae.configure_optimizers()

    def ae_step():
        opt.zero_grad(set_to_none=True)
        ae.training_step(batch, 0).backward()
        opt.step()

    d = time_steps(ae_step, 5, 2)
    out["flow_autoencoder"] = {"workload": "LitAutoEncoder train step (notebook 13), [64,2,5,128,128] -> [64,1,1,64,64], f32",
                               "ms_per_step": round(d * 1e3, 2), "samples_per_s": round(b / d, 1),
                               "tflops_f32": round(3 * 2 * 1.097e9 * b / d / 1e12, 1)}
    del ae, opt, batch

    from predict_pv_yield_amd.data.fake import FakeDataConfiguration, make_fake_batch
    from predict_pv_yield_amd.models.perceiver.perceiver import PerceiverModel
    b = 8
    cfg = FakeDataConfiguration(batch_size=b, history_minutes=60, forecast_minutes=30, satellite_image_size_pixels=64,
                                nwp_image_size_pixels=64)
    pbatch = make_fake_batch(cfg, torch.Generator().manual_seed(2)).to(dev)
    out["perceiver"] = {"workload": "PerceiverModel train step (configs/model/perceiver.yaml): B=8, T=19 frames = 19 weight-tied "
                                    "layers, 64x64x11, 128 latents x 64"}
    for dt in ("f32", "bf16"):
        torch.manual_seed(0)
        pm = PerceiverModel(history_minutes=60, forecast_minutes=30, batch_size=b, num_latents=128, latent_dim=64,
                            embedding_dem=16, output_variable="gsp_yield", operand_dtype=dt).to(dev)
        popt = pm.configure_optimizers()

        def p_step():
            popt.zero_grad(set_to_none=True)
            pm.training_step(pbatch, 0).backward()
            popt.step()

        d = time_steps(p_step, 3, 1)
        out["perceiver"][f"attention_operands_{dt}"] = {"ms_per_step": round(d * 1e3, 1), "samples_per_s": round(b / d, 1)}
        del pm, popt
        settle()
    del pbatch

    # BASELINE configs[4]: experiments/003 LitModel, 128 x 128 x 12 images (16 384-position context), NWP, precision 16
    from predict_pv_yield_amd.models.perceiver.exp003 import LitModel, make_fake_exp003_batch
    b = 8
    ebatch = {k: v.to(dev) for k, v in make_fake_exp003_batch(b, 128, torch.Generator().manual_seed(3)).items()}
    out["exp003_perceiver_rnn"] = {"workload": f"experiments/003 LitModel train step: B={b} x 19 images of 128x128x12 (context 16384 "
                                               "positions x 38 ch), Perceiver depth 2 (128 latents x 64) -> fc -> 2-layer GRU "
                                               "encoder / decoder with NWP + datetime features"}
    n_frames, n_k = b * 19, 128 * 128
    fwd_flop = 2 * 2.0 * n_frames * 128 * n_k * 64          # q k^T and p v of one cross-attention launch
    for dt in ("f32", "bf16"):
        torch.manual_seed(0)
        em = LitModel(operand_dtype=dt).to(dev)
        eopt = em.configure_optimizers()

        def e_step():
            eopt.zero_grad(set_to_none=True)
            em.training_step(ebatch, 0).backward()
            eopt.step()

        d = time_steps(e_step, 10, 5)      # (the first steps of a process also pay workspace and allocator growth)
        entry = {"ms_per_step": round(d * 1e3, 2), "samples_per_s": round(b / d, 1)}
        with LaunchTimer(("attention_fwd", "attention_bwd")) as lt:
            for _ in range(2):
                e_step()
        peak = MFMA_BF16_PEAK if dt == "bf16" else MFMA_F32_PEAK
        per = {}
        for (name, shape, _), (secs, n) in lt.summary().items():
            per.setdefault(name, []).append((secs, n))
        for name, lst in per.items():
            secs = max(s_ for s_, _ in lst)                 # the cross-attention launches (16 384 keys) are the long ones
            fl = fwd_flop * (1.0 if name == "attention_fwd" else 2.5)
            entry[f"cross_{name}"] = {"us_per_launch": round(secs * 1e6, 1), "tflops": round(fl / secs / 1e12, 1),
                                      "frac_of_peak": round(fl / secs / peak, 4),
                                      "peak": "bf16 dense 2.5 PF" if dt == "bf16" else "f32 matrix 157 TF"}
        out["exp003_perceiver_rnn"][f"attention_operands_{dt}"] = entry
        del em, eopt
        settle()
    # the same step (bf16 operands) replayed as ONE HIP graph: ~600 launches per step keep the host as busy as the device in
    # eager mode (graphs.GraphedTrainStep; losses identical to the eager step: tests/test_gpu_exp003.py)
    try:
        from predict_pv_yield_amd.graphs import GraphedTrainStep
        from predict_pv_yield_amd.optim import HipAdam
        torch.manual_seed(0)
        em = LitModel(operand_dtype="bf16").to(dev)
        gstep = GraphedTrainStep(em, HipAdam(em.parameters(), lr=0.0005, capturable=True), ebatch, warmup=3)
        d = time_steps(lambda: gstep(ebatch), 8, 3)
        out["exp003_perceiver_rnn"]["attention_operands_bf16"]["hip_graph_ms_per_step"] = round(d * 1e3, 2)
        gstep.close()
        del em, gstep
    except Exception as e:      # noqa: BLE001 -- a secondary figure must not take the bench line down
        out["exp003_perceiver_rnn"]["attention_operands_bf16"]["hip_graph_ms_per_step"] = f"failed: {type(e).__name__}: {e}"
    settle()
    return out


# ------------------------------------------------------------------------------------------------------------------
# matched validation NMAE + CPU baseline: the torch-CPU oracle's train steps serve both
# ------------------------------------------------------------------------------------------------------------------
def learnable_task_on_device(n, t_frames, gen, dev):
    """Synthetic but learnable, generated on the device (26 M normals per batch take the host 0.15 s and the device 0.1 ms): every
    sample carries a brightness offset (a stand-in for cloud cover) on three channels of its observed frames, and the PV yield
    of the 6 forecast steps is a smooth function of it."""
    sat = torch.randn(n, 11, t_frames, 64, 64, generator=gen, device=dev)
    level = torch.rand(n, generator=gen, device=dev) * 2.0 - 1.0
    sat[:, :3, : t_frames - 6] += level[:, None, None, None, None]
    pv = torch.rand(n, t_frames, 128, generator=gen, device=dev)
    steps = torch.arange(6, dtype=torch.float32, device=dev)
    pv[:, -6:, 0] = torch.sigmoid(2.0 * level[:, None] + 0.2 * steps[None])
    return sat, pv


# Gate of the matched-validation experiment (round 6, VERDICT r5 item 4: the round-5 gate max(2e-3, 2 s.e.) WIDENED with the
# noise of the run; SURVEY section 8c asks for "matched validation NMAE" at 1e-3 .. 2e-3 absolute):
#   |mean over seeds of the paired difference (bf16 - fp32)| <= 2e-3   AND   its standard error <= 7e-4,
# seeds added in blocks of VAL_SEED_BLOCK until the second clause holds (or VAL_SEEDS_MAX is reached: then the gate FAILS --
# an estimate that noisy decides nothing)
VAL_GATE_ABS, VAL_GATE_SE_MAX = 2e-3, 7e-4
VAL_SEED_BLOCK, VAL_SEEDS_MAX = 8, 48


def matched_validation_and_cpu_baseline(dev, history_minutes, seeds=None, n_steps=512, batch=32, n_val=1024, tail=64, tail_stride=4,
                                        oracle_seconds=30.0, early=8):
    """"At matched validation NMAE" with statistical power, and the CPU baseline from the same oracle steps.

    Per seed: ONE set of initial weights and ONE sequence of batches (B = 32, the benched batch) of the learnable synthetic
    task; the HIP bf16 model (the benched path) and the HIP fp32 model (the rtol 1e-4 parity path) each take n_steps Adam steps
    on them; the figure of a run is its validation NMAE on n_val held-out samples AVERAGED OVER THE LAST `tail` STEPS (every
    tail_stride-th of them; a single checkpoint swings by sigma ~ 0.02 under Adam(5e-4) on 128 M weights: 64 steps at B = 8 on
    256 samples -- round 4 -- was a noise experiment).  The two runs of a seed share weights and batches, so the statistic is
    the PAIRED difference bf16 - fp32 over the seeds, with its standard error.
    The torch-CPU oracle (oracle/conv3d_oracle.py: the reference's arithmetic, identical to its Lightning path) follows seed 0
    from the same weights on the same batches for as many steps as `oracle_seconds` allow: its train steps are timed (that is
    cpu_baseline, at the benched batch), its first-steps train losses are compared with the two HIP runs' (an arithmetic
    regression shows there first), and its last checkpoint is scored twice -- by the oracle on the CPU and through the HIP fp32
    forward (same weights, two scorers)."""
    import statistics
    from oracle import conv3d_oracle as co
    from predict_pv_yield_amd.models.conv3d.model import Model
    t_frames = 18 if history_minutes == 55 else 19
    models = {}
    for prec in ("fp32", "bf16"):
        m = Model(**MODEL_KW, history_minutes=history_minutes, precision=prec).to(dev)
        m.batch_size = max(m.batch_size, n_val, batch)
        models[prec] = m
    vgen = torch.Generator(device=dev).manual_seed(77)
    val_sat, val_pv = learnable_task_on_device(n_val, t_frames, vgen, dev)
    y_val = val_pv[:, -6:, 0]

    def hip_val(m, n=n_val):
        with torch.no_grad():
            ys = [m({"satellite": {"data": val_sat[i:i + 64]}, "pv": {"pv_yield": val_pv[i:i + 64]}}) for i in range(0, n, 64)]
        return float((torch.cat(ys) - y_val[:n]).abs().mean())

    def reinitialise(m, seed):      # torch's default initialisation (U(-1/sqrt(fan_in), 1/sqrt(fan_in)) for weights and biases), on the device
        g = torch.Generator(device=dev).manual_seed(518 + 1000 * seed)
        with torch.no_grad():
            for _, mod in m.named_modules():
                w = getattr(mod, "weight", None)
                if w is None or not isinstance(w, torch.nn.Parameter):
                    continue
                bound = 1.0 / w[0].numel() ** 0.5
                w.uniform_(-bound, bound, generator=g)
                if getattr(mod, "bias", None) is not None:
                    mod.bias.uniform_(-bound, bound, generator=g)

    def batches_of(seed, n=n_steps):
        g = torch.Generator(device=dev).manual_seed(100 + 1000 * seed)
        for _ in range(n):
            yield learnable_task_on_device(batch, t_frames, g, dev)

    tail_steps = set(range(n_steps, n_steps - tail, -tail_stride))
    runs = {"bf16": [], "fp32": []}
    early_loss = {"bf16": [], "fp32": []}
    t_hip = time.perf_counter()
    init0 = None
    se = lambda v: statistics.stdev(v) / len(v) ** 0.5 if len(v) > 1 else float("nan")
    seed = -1
    while True:
        seed += 1
        if seeds is not None:
            if seed >= seeds:
                break
        elif seed and seed % VAL_SEED_BLOCK == 0:
            # sequential rule, fixed beforehand: stop at the first block boundary where the paired difference's standard
            # error is below the gate's bound (the MEAN is not looked at), or at VAL_SEEDS_MAX
            if se([a - b for a, b in zip(runs["bf16"], runs["fp32"])]) <= VAL_GATE_SE_MAX or seed >= VAL_SEEDS_MAX:
                break
        reinitialise(models["fp32"], seed)
        init = {k: v.clone() for k, v in models["fp32"].state_dict().items()}      # reference layout (the state-dict hook's)
        if seed == 0:
            init0 = {k: v.cpu() for k, v in init.items()}
        for prec in ("bf16", "fp32"):
            m = models[prec]
            m.load_state_dict(init)
            opt = m.configure_optimizers()
            acc = []
            for i, (sat, pv) in enumerate(batches_of(seed)):
                opt.zero_grad(set_to_none=True)
                loss = m.training_step({"satellite": {"data": sat}, "pv": {"pv_yield": pv}}, 0)
                loss.backward()
                opt.step()
                if seed == 0 and i < early:
                    early_loss[prec].append(float(loss.detach()))
                if i + 1 in tail_steps:
                    acc.append(hip_val(m))
            runs[prec].append(sum(acc) / len(acc))
            del opt
            settle()
    t_hip = time.perf_counter() - t_hip
    diffs = [a - b for a, b in zip(runs["bf16"], runs["fp32"])]
    seeds = len(diffs)
    d_mean, d_se = statistics.fmean(diffs), se(diffs)

    # ---- the CPU oracle on seed 0's weights and batches: timed train steps, first-steps losses, last checkpoint ----------
    oracle = co.OracleConv3dModel(**MODEL_KW, history_minutes=history_minutes)
    oracle.load_state_dict(init0)
    ref_opt = co.make_optimizer(oracle)
    all_threads = torch.get_num_threads()
    plans = sorted({all_threads, max(1, all_threads // 4)}, reverse=True)   # oneDNN's Conv3d does not always scale to every thread
    rates, o_loss, done, t_start = {}, [], 0, time.perf_counter()
    host_batches = batches_of(0)

    def oracle_step(threads, record=True):
        nonlocal done
        sat, pv = next(host_batches)
        sat, pv = sat.cpu(), pv.cpu()
        torch.set_num_threads(threads)
        t0 = time.perf_counter()
        o_loss.append(co.train_steps(oracle, sat, pv, 1, ref_opt)[0])
        dt = time.perf_counter() - t0
        done += 1
        if record:
            acc = rates.setdefault(threads, [0.0, 0])
            acc[0] += dt
            acc[1] += 1

    oracle_step(plans[0], record=False)                     # first step: one-time oneDNN primitive creation
    for threads in plans:
        oracle_step(threads)
    best_threads = max(plans, key=lambda th: rates[th][1] / rates[th][0])
    while time.perf_counter() - t_start < oracle_seconds and done < n_steps:
        oracle_step(best_threads)
    torch.set_num_threads(all_threads)
    rate = {th: round(n * batch / sec, 2) for th, (sec, n) in rates.items()}
    train_s = sum(sec for sec, _ in rates.values())
    # same weights, two scorers: the oracle's own forward on the CPU (256 samples: ~2 s) and the HIP fp32 forward
    models["fp32"].load_state_dict(oracle.state_dict())
    via_hip = hip_val(models["fp32"], 256)
    with torch.no_grad():
        vs, vp = val_sat[:256].cpu(), val_pv[:256].cpu()
        own = float((torch.cat([oracle(vs[i:i + 32]) for i in range(0, 256, 32)]) - vp[:, -6:, 0]).abs().mean())
    same_w = abs(own - via_hip) / own
    rel = lambda a, b: max(abs(x - y) / abs(y) for x, y in zip(a, b))
    n_early = min(early, done)
    early_cmp = {"steps": n_early, "train_nmae_oracle": [round(v, 6) for v in o_loss[:n_early]],
                 "train_nmae_hip_fp32": [round(v, 6) for v in early_loss["fp32"][:n_early]],
                 "train_nmae_hip_bf16": [round(v, 6) for v in early_loss["bf16"][:n_early]],
                 "first_4_steps_hip_fp32_vs_oracle": round(rel(early_loss["fp32"][:4], o_loss[:4]), 6),
                 "max_rel_diff_hip_fp32_vs_oracle": round(rel(early_loss["fp32"][:n_early], o_loss[:n_early]), 5),
                 "step_1_hip_bf16_vs_oracle": round(rel(early_loss["bf16"][:1], o_loss[:1]), 7),
                 "step_2_hip_bf16_vs_oracle": round(rel(early_loss["bf16"][1:2], o_loss[1:2]), 6),
                 "note": "same weights, same batches (B = 32): step 1 compares forwards on identical weights; from step 2 on Adam's "
                         "first updates (lr x sign of the gradient for every one of 128 M weights) turn bf16 rounding of near-zero "
                         "gradients into whole steps of opposite sign; the two f32 sides differ by summation order only"}
    val = {"definition": f"validation NMAE on {n_val} held-out samples, mean over every {tail_stride}th of the last {tail} of {n_steps} Adam "
                         f"steps at B = {batch}; {seeds} seeds (initial weights + batches; blocks of {VAL_SEED_BLOCK} until the paired "
                         f"difference's standard error is <= {VAL_GATE_SE_MAX}, at most {VAL_SEEDS_MAX}), the bf16 and the fp32 run of a seed share both",
           "n_seeds": seeds,
           "hip_bf16": round(statistics.fmean(runs["bf16"]), 6), "hip_fp32": round(statistics.fmean(runs["fp32"]), 6),
           "seeds": {"hip_bf16": {"runs": [round(v, 5) for v in runs["bf16"]], "standard_error": round(se(runs["bf16"]), 5)},
                     "hip_fp32": {"runs": [round(v, 5) for v in runs["fp32"]], "standard_error": round(se(runs["fp32"]), 5)}},
           "paired_bf16_minus_fp32": {"per_seed": [round(v, 5) for v in diffs], "mean": round(d_mean, 5), "standard_error": round(d_se, 5),
                                      "in_standard_errors": round(abs(d_mean) / d_se, 2) if d_se > 0 else None},
           "gate": {"abs_mean_at_most": VAL_GATE_ABS, "standard_error_at_most": VAL_GATE_SE_MAX,
                    "rule": "both clauses; seeds are added until the second holds, the mean is not looked at while adding"},
           "early_train_loss": early_cmp,
           "same_weights_rel_diff": round(same_w, 7),
           "oracle_seed0": {"steps_in_budget": done, "train_seconds": round(train_s, 1)},
           "hip_seconds": round(t_hip, 1),
           "task": "BASELINE config 2 model (T=18, 64 px, fc 128/128/64); every sample has a brightness offset u ~ U(-1, 1) on 3 "
                   "channels of its observed frames, yield = sigmoid(2 u + 0.2 step)"}
    # bounds of the first-steps comparison: about twice what the committed collection shows (profiles/r05/NOTES.md); the kernels
    # are deterministic, so these figures repeat to the digit on a given input.  A bf16 path that lost a further bit of operand
    # precision doubles its step-2 figure; an f32 path that lost accumulation precision breaks the f32 bounds; a forward that
    # drifted from the oracle's breaks step 1 and the same-weights bound
    checks = {f"|mean paired bf16 - fp32| <= {VAL_GATE_ABS}": abs(d_mean) <= VAL_GATE_ABS,
              f"standard error of the paired difference <= {VAL_GATE_SE_MAX}": d_se <= VAL_GATE_SE_MAX,
              "early_loss_first_4_steps_hip_fp32_vs_oracle <= 2e-4": early_cmp["first_4_steps_hip_fp32_vs_oracle"] <= 2e-4,
              "early_loss_step_1_hip_bf16_vs_oracle <= 2e-5": early_cmp["step_1_hip_bf16_vs_oracle"] <= 2e-5,
              "early_loss_step_2_hip_bf16_vs_oracle <= 1.2e-2": early_cmp["step_2_hip_bf16_vs_oracle"] <= 1.2e-2,
              "same_weights_two_scorers <= 1e-4": same_w <= 1e-4}
    val["checks"], val["pass"] = checks, all(checks.values())
    cpu = {"value": rate[best_threads], "unit": "samples/s", "cores": best_threads, "kind": "port",
           "sample": f"{done} Adam steps at B={batch} (the benched batch), T={t_frames}, fp32, torch-CPU oracle (oracle/conv3d_oracle.py: "
                     f"the reference's Conv3D / fc / NMAE / Adam operators), {train_s:.1f} s of train steps; samples/s by thread count {rate}"}
    del models, oracle, val_sat, val_pv
    settle()
    return val, cpu


def flow_cpu_baseline(n_single=4, per_thread=2):
    """The advection pipeline of config 3 on the host: oracle/pv_oracle.c (the restatement of cv.calcOpticalFlowFarneback /
    cv.remap; OpenCV itself is not installable here) on the same [12, 11, 64, 64] count stacks, 121 Farneback pairs per
    sample.  One thread, and one stack per hardware thread in a thread pool (the C library runs with the GIL released; the
    reference fans the pairs of a stack out over a process pool, notebooks/13_...ipynb:202-232)."""
    import concurrent.futures as cf
    import numpy as np
    from oracle import flow_oracle as fo
    from predict_pv_yield_amd import optical_flow as of
    from predict_pv_yield_amd.data.synthetic import advected_counts
    mean, std = of.SAT_MEAN[1:12], of.SAT_STD[1:12]
    threads = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    raw, _ = advected_counts(batch=max(n_single, min(threads * per_thread, 256)), t=12, channels=11, h=64, w=64, seed=1234)
    one = lambda i: fo.advect_frames(raw[i:i + 1], mean, std, n_future=6)
    one(0)
    t0 = time.perf_counter()
    for i in range(n_single):
        one(i)
    single = n_single / (time.perf_counter() - t0)
    n_pool = min(threads * per_thread, raw.shape[0])
    with cf.ThreadPoolExecutor(max_workers=threads) as pool:
        t0 = time.perf_counter()
        list(pool.map(one, range(n_pool)))
        pooled = n_pool / (time.perf_counter() - t0)
    return {"kind": "port", "unit": "samples/s (121 Farneback pairs + weighted mean + normalise + 6 remaps per sample)",
            "one_thread": {"samples_per_s": round(single, 2), "pairs_per_s": round(121 * single, 1), "ms_per_pair": round(1e3 / (121 * single), 3)},
            "all_threads": {"samples_per_s": round(pooled, 2), "pairs_per_s": round(121 * pooled, 1), "cores": threads,
                            "sample": f"{n_pool} stacks in a pool of {threads} threads"},
            "reference_figure": "cv.calcOpticalFlowFarneback on the 704 x 548 frames of the notebook: ~173 ms per pair on its "
                                "author's CPU (notebooks/optical_flow_1.ipynb:269) = 2.2 Mpx/s; a 64 x 64 tile is 1/94 of that frame"}


class ClockSampler:
    """Samples the amdgpu driver's current engine / memory clock levels (sysfs pp_dpm_sclk / pp_dpm_mclk: the line marked '*')
    and the board power from a host thread while the timed steps run -- no device work, no HIP call.  The same binary steps
    in 1.54 ms on one box of the pool and 1.71 ms on another (fc1's HBM-bound backward 0.64 against 0.78 ms); the clocks the
    device held under THIS load are logged beside the bench line so that a slow box can be told from a slow kernel.  The
    box may expose several cards while one is visible to the process: the card with the highest median engine clock during the
    run is taken to be the one under load."""

    def __init__(self, period_s=0.01):
        import glob
        self.period = period_s
        self.cards = sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk"))
        self.samples = {c: {"sclk": [], "mclk": [], "fclk": [], "power": [], "sclk_now": [], "temp": []} for c in self.cards}
        # hwmon: freq1_input = the engine clock the device is running at NOW (Hz; the pp_dpm level is the state it was asked for),
        # power1_average or power1_input (uW), the hottest temp*_input (millidegrees)
        self.hwmon = {}
        for c in self.cards:
            d = os.path.dirname(c)
            hw = (glob.glob(os.path.join(d, "hwmon", "hwmon*")) + [None])[0]
            files = {}
            if hw:
                for key, names in (("sclk_now", ("freq1_input",)), ("power", ("power1_average", "power1_input"))):
                    for nme in names:
                        if os.path.exists(os.path.join(hw, nme)):
                            files[key] = os.path.join(hw, nme)
                            break
                files["temps"] = sorted(glob.glob(os.path.join(hw, "temp*_input")))
            self.hwmon[c] = files
        self._stop = None

    @staticmethod
    def _read_int(path):
        try:
            return int(open(path).read())
        except Exception:      # noqa: BLE001 -- absent or unreadable: no sample
            return None

    @staticmethod
    def _active_mhz(path):
        try:
            for ln in open(path).read().splitlines():
                if ln.rstrip().endswith("*"):
                    return int("".join(ch for ch in ln.split(":")[1] if ch.isdigit()))
        except Exception:      # noqa: BLE001 -- sysfs absent or unreadable: no sample
            pass
        return None

    def __enter__(self):
        import threading
        self._stop = threading.Event()

        def loop():
            import glob
            while not self._stop.is_set():
                for c in self.cards:
                    d = os.path.dirname(c)
                    s_, m_ = self._active_mhz(c), self._active_mhz(os.path.join(d, "pp_dpm_mclk"))
                    if s_ is not None:
                        self.samples[c]["sclk"].append(s_)
                    if m_ is not None:
                        self.samples[c]["mclk"].append(m_)
                    f_ = self._active_mhz(os.path.join(d, "pp_dpm_fclk"))
                    if f_ is not None:
                        self.samples[c]["fclk"].append(f_)
                    hw = self.hwmon.get(c, {})
                    v = self._read_int(hw["sclk_now"]) if "sclk_now" in hw else None
                    if v is not None:
                        self.samples[c]["sclk_now"].append(round(v / 1e6))
                    v = self._read_int(hw["power"]) if "power" in hw else None
                    if v is not None:
                        self.samples[c]["power"].append(v / 1e6)
                    ts = [t for t in (self._read_int(tp) for tp in hw.get("temps", [])) if t is not None]
                    if ts:
                        self.samples[c]["temp"].append(max(ts) / 1e3)
                self._stop.wait(self.period)

        self._thread = threading.Thread(target=loop, daemon=True)
        self._thread.start()
        return self

    def __exit__(self, *exc):
        self._stop.set()
        self._thread.join(timeout=2.0)
        return False

    def summary(self):
        import statistics
        best, best_key = None, (-1, -1)
        for c, smp in self.samples.items():      # the card under load: the highest median power, then engine clock
            if smp["sclk"]:
                key = (statistics.median(smp["power"]) if smp["power"] else -1, statistics.median(smp["sclk"]))
                if key > best_key:
                    best, best_key = c, key
        if best is None:
            return {"available": False}
        smp = self.samples[best]
        q = lambda v: {"min": min(v), "median": statistics.median(v), "max": max(v)} if v else None
        return {"available": True, "card": best.split("/")[4], "cards_seen": len(self.cards), "samples": len(smp["sclk"]),
                "sclk_MHz": q(smp["sclk"]), "sclk_now_MHz": q(smp["sclk_now"]), "mclk_MHz": q(smp["mclk"]), "fclk_MHz": q(smp["fclk"]),
                "power_W": q([round(x, 1) for x in smp["power"]]), "hottest_sensor_C": q([round(x, 1) for x in smp["temp"]]),
                "source": "sysfs pp_dpm_sclk / _mclk / _fclk (active level), hwmon freq1_input (engine clock now), power1_*, temp*_input; "
                          "sampled every 10 ms during the timed steps"}


def exchange_bytes(mode, world, b, model):
    """Bytes one rank SENDS per step for fc1 under each exchange (the small tensors' flat bucket, ~0.6 MB, is the same in all)."""
    n, k = model.fc1.weight.shape
    f = (world - 1) / world
    if mode == "ksharded":
        return {"all_to_all_activations_bf16": int(b * k * 2 * f), "all_to_all_input_gradient_bf16": int(b * k * 2 * f),
                "partial_outputs_f32": int(world * b * n * 4 * f), "all_gather_output_gradient_f32": int(b * n * 4 * (world - 1))}
    if mode == "sharded":
        return {"reduce_scatter_gradient_bf16": int(n * k * 2 * f), "all_gather_operand_copy_bf16": int(n * k * 2 * f)}
    if mode == "bf16":
        return {"all_reduce_gradient_bf16": int(2 * n * k * 2 * f)}
    return {"all_reduce_gradient_f32": int(2 * n * k * 4 * f)}


def collectives_info(world, requested, in_force):
    """What the job's exchange really ran on, read from the live process group: the first 8-GPU run certifies itself."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return {"backend": None, "world_size": world}
    info = {"backend": dist.get_backend(), "world_size": dist.get_world_size(), "requested_mode": requested, "mode_in_force": in_force,
            "visible_devices": torch.cuda.device_count()}
    try:
        info["rccl_version"] = ".".join(str(v) for v in torch.cuda.nccl.version())
    except Exception as e:      # noqa: BLE001
        info["rccl_version"] = f"unavailable ({type(e).__name__})"
    for k in ("NCCL_DEBUG", "HSA_ENABLE_IPC_MODE_LEGACY", "PV_DIST_BACKEND", "PV_SINGLE_DEVICE"):
        if k in os.environ:
            info[k] = os.environ[k]
    return info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # defaults: long enough for the device to settle (same box, alternating: W=5 / K=20 reads 1.744-1.758 ms, W=40 / K=100 and
    # W=100 / K=200 read 1.716-1.728 ms) and still a fraction of a second of timed work
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--batch", type=int, default=32, help="per-GPU batch of PV-site crop stacks")
    ap.add_argument("--global-batch", type=int, default=0,
                    help="strong scaling: fix the GLOBAL batch (e.g. 512) and give each of the N GPUs global/N samples; "
                         "default 0 = weak scaling with --batch samples per GPU")
    ap.add_argument("--history-minutes", type=int, default=55, help="55 -> T=18 (12 observed + 6 forecast frames)")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: device calibration, clocks during the timed steps, the other fc1 exchanges "
                         "(N > 1), roofline, config 3, fp32, other models, sweeps, matched validation and the CPU baselines "
                         "(N = 1); the --no-* options below trim this set")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write the last step's loss and the parameters it left as float32 DIR/<name>.npy "
                         "(fc1.weight as a fixed, seeded sample)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU leg (matched training + cpu_baseline)")
    ap.add_argument("--no-roofline", action="store_true", help="--full: skip every secondary GPU leg")
    ap.add_argument("--no-extras", action="store_true", help="--full: keep roofline but skip config 3, fp32 and the other models")
    ap.add_argument("--no-calibration", action="store_true", help="--full: skip the in-process device calibration before the timed steps")
    ap.add_argument("--overlap-update", action="store_true",
                    help="N = 1: launch fc1's fused wgrad+Adam from backward on a side stream (under the conv backward)")
    ap.add_argument("--f32-grads", action="store_true", help="N > 1: all-reduce fc1's gradient in f32 instead of bf16")
    ap.add_argument("--grad-sync", choices=["auto", "sharded", "allreduce", "ksharded"], default="auto",
                    help="N > 1, bf16 gradients: 'ksharded' = fc1's columns dealt over the ranks, activations exchanged by two "
                         "all-to-alls (no weight or gradient of fc1 crosses a link: 0.45 GB per rank and step at 8 x 64 samples "
                         "where the row-sharded form sends 1.03 GB, and one rank's kernels are the faster of the two); 'sharded' = "
                         "reduce-scatter + per-rank Adam over its rows of fc1 + all-gather of the bf16 operand copy; 'allreduce' = "
                         "every rank steps the whole matrix.  'auto' (default): the first of ksharded / sharded / bf16 all-reduce / "
                         "f32 all-reduce whose trial step succeeds on every rank -- the line names the mode in force "
                         "(config.parallelism, config.collectives); a mode asked for BY NAME is never replaced (exit non-zero "
                         "instead, unless --allow-demotion)")
    ap.add_argument("--only-requested-mode", action="store_true",
                    help="N > 1, --full: time the requested exchange only (otherwise the other modes are timed afterwards in the "
                         "same invocation and reported under grad_sync_modes; `value` is always the requested mode's)")
    ap.add_argument("--other-modes-budget", type=float, default=float(os.environ.get("PV_BENCH_OTHER_MODES_BUDGET_S", "120")),
                    help="N > 1: seconds the leg that times the OTHER fc1 exchanges may take; past it the requested mode's line is "
                         "printed with what the leg has recorded and the process ends (a collective one rank never enters cannot be interrupted)")
    ap.add_argument("--allow-demotion", action="store_true",
                    help="N > 1: accept a simpler gradient-exchange mode than the requested one when its trial step fails "
                         "(default: exit non-zero -- a scaling number on another exchange is not the number asked for)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    from predict_pv_yield_amd import distributed as D
    from predict_pv_yield_amd.models.conv3d.model import Model

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (the product has no CPU path)")
    distributed = D.init_from_env()
    world = torch.distributed.get_world_size() if distributed else 1
    rank = torch.distributed.get_rank() if distributed else 0
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus}")
    dev = torch.device("cuda", D.local_device_index())
    torch.cuda.set_device(dev)

    model_kwargs = dict(MODEL_KW, history_minutes=args.history_minutes, precision=args.precision)
    torch.manual_seed(518)  # configs/experiment/conv3d.yaml:16
    model = Model(**model_kwargs).to(dev)
    t_frames = model.history_len_5 + model.forecast_len_5 + 1
    if distributed:
        D.broadcast_parameters(model)
    opt = model.configure_optimizers()
    opt.grad_scale = 1.0 / world
    if args.overlap_update and not distributed:
        opt.overlap_large_update = True
        opt.set_large_grad_mode("fused")

    g = torch.Generator(device=dev).manual_seed(518 + rank)
    b = args.batch
    if args.global_batch:
        if args.global_batch % world:
            raise SystemExit("--global-batch must be a multiple of the number of GPUs")
        lo, hi = D.shard_range(args.global_batch)      # this rank's samples of the global batch (contiguous, equal counts)
        b = hi - lo
    model.batch_size = max(model.batch_size, b)  # BaseModel.batch_size slices the target (base_model.py:95)
    batch = {"satellite": {"data": torch.randn(b, 11, t_frames, 64, 64, generator=g, device=dev)},
             "pv": {"pv_yield": torch.rand(b, t_frames, 128, generator=g, device=dev)}}

    sync = None
    grad_sync_mode = None
    if distributed:
        # the exchange needs a materialised fc1 gradient: bf16 on the wire (half the xGMI bytes), f32 with --f32-grads.
        # The row-sharded exchange (reduce-scatter / all-gather) is tried ONCE, untimed, in this process; if RCCL refuses
        # it on every rank alike the run continues on the plain bf16 all-reduce (never a re-exec: the GPU is initialised).
        grad_sync_mode = "autograd" if args.f32_grads else {"auto": "ksharded", "sharded": "sharded", "allreduce": "bf16",
                                                            "ksharded": "ksharded"}[args.grad_sync]
        auto = args.grad_sync == "auto" and not args.f32_grads
        requested_mode = "auto (ksharded, sharded, bf16, autograd: the first whose trial step succeeds)" if auto else grad_sync_mode
        grad_sync_mode = D.negotiate_grad_sync(model, opt, batch, grad_sync_mode, allow_demotion=args.allow_demotion or auto)
        sync = D.OverlappedGradSync(model)

    from predict_pv_yield_amd.lightning import Trainer

    def step():
        opt.zero_grad(set_to_none=True)
        loss = model.training_step(batch, 0)
        Trainer._backward(loss)      # = loss.backward() as the Trainer issues it; under N > 1 fc1's exchange starts inside
        if sync is not None:
            sync.finish()
        opt.step()
        return loss

    first = None
    for i in range(args.warmup):
        l = step()
        if i == 0:
            first = float(l.detach())
    # what THIS device sustains (copy rate, bare bf16 matrix-instruction rate), in this process, right before the timed steps:
    # one binary runs 1.52-1.71 ms per step across a pool's boxes, so fractions are reported against the spec peaks AND these
    calibration = None
    if args.full and args.warmup > 0 and not args.no_calibration:
        from predict_pv_yield_amd import hip_ops as K
        calibration = K.device_calibration()
        for _ in range(3):          # back into the step's own rhythm (allocator, clocks) before timing
            step()
    if distributed:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    clocks = ClockSampler() if args.full else None
    with clocks or contextlib.nullcontext():
        t0 = time.perf_counter()
        for _ in range(args.steps):
            last = step()
        torch.cuda.synchronize()
        if distributed:
            torch.distributed.barrier()
        elapsed = time.perf_counter() - t0
    if distributed:
        tt = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        torch.distributed.all_reduce(tt, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(tt.item())
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, model, opt, last, distributed, rank)
    last = float(last.detach())

    # N > 1: the other exchanges of fc1, timed the same way in the SAME invocation (the first multi-GPU run
    # decides between exchanges instead of testing one).  Every rank walks the same list; a mode whose trial step fails, or that
    # the optimiser replaces by a simpler one, is recorded as such and skipped -- `value` above stays the requested mode's.
    other_modes = {}
    distributed_roofline = {}
    headline = None
    if rank == 0:      # the requested mode's own result: everything below adds to it, nothing below may lose it
        value = world * b * args.steps / elapsed
        ms_step = elapsed / args.steps * 1e3
        headline = {
            "metric": "PV-site samples/sec (train step), conv3d 12->6 frames",
            "value": round(value, 2), "unit": "samples/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(ms_step, 3), "higher_is_better": True,
            "scaling": "strong" if args.global_batch else "weak", "vs_baseline": None, "dtype": args.precision, "data": "synthetic",
            "config": {"workload": f"conv3d train step (fwd + NMAE + bwd + Adam): sat [B,11,{t_frames},64,64] N(0,1), "
                                   f"4x Conv3d(3x3x3, 32ch) + fc 128/128/64, {sum(p.numel() for p in model.parameters())/1e6:.1f} M params",
                       "per_gpu_batch": b, "global_batch": b * world, "t_frames": t_frames,
                       "parallelism": f"dp{world} ({grad_sync_mode})" if world > 1 else "single",
                       "collectives": collectives_info(world, requested_mode if distributed else None, grad_sync_mode)},
            "device_calibration": calibration,
            "device_clocks_during_timed_steps": clocks.summary() if clocks else None,
        }

    def modes_record():
        if not distributed:
            return None
        return dict({grad_sync_mode: {"status": "ok (the requested mode: `value`)", "ms_per_step": headline["ms_per_step"],
                                      "value": headline["value"], "unit": "samples/s",
                                      "collectives": collectives_info(world, requested_mode, grad_sync_mode),
                                      "exchange_bytes_per_rank_and_step": exchange_bytes(grad_sync_mode, world, b, model)}},
                    **other_modes)

    if distributed and args.full and not args.only_requested_mode:
        # A collective that one rank never enters cannot be interrupted from inside: a timer thread prints the requested mode's
        # line with what the leg has recorded so far and ends the process (exit code 0 -- `value` was measured; never an exec).
        import threading
        current = {"mode": None}

        def leg_expired():
            if rank == 0:
                other_modes.setdefault(current["mode"] or "?", {"status": f"no answer within {args.other_modes_budget:.0f} s: leg abandoned"})
                line = dict(headline, grad_sync_modes=modes_record(), train_nmae_first_step=first, train_nmae_last_step=last,
                            roofline=distributed_roofline or None, cpu_baseline=None)
                print(json.dumps(line), flush=True)
            else:
                time.sleep(2.0)      # (rank 0 prints first)
            os._exit(0)
        watchdog = threading.Timer(args.other_modes_budget, leg_expired)
        watchdog.daemon = True
        watchdog.start()

        # the roofline object of the line under N > 1 (mode in force, before the other modes are tried): rank 0 brackets its
        # launches with HIP events over six more steps while every rank takes the same six.  fc1's pass is a 1 / N shard here:
        # the step's dominant family is the 32 -> 32 conv forward / dgrad kernels, priced against the matrix peak
        if args.precision == "bf16" and not args.no_roofline:
            current["mode"] = "roofline leg of the mode in force"
            if rank == 0:
                try:
                    roof = measure_step_rooflines(step, model, b, t_frames)
                    if "bound" not in roof and "mfma_conv3d" in roof:
                        fam = roof.pop("mfma_conv3d")
                        roof = dict(fam, **roof)
                    distributed_roofline.update(roof)
                except Exception as e:      # noqa: BLE001 -- (a failure between two steps leaves the ranks out of step: the timer ends the leg)
                    distributed_roofline.update({"error": f"{type(e).__name__}: {e}"})
                    watchdog.join()
            else:
                for _ in range(6):
                    step()
            torch.distributed.barrier()

        def timed_steps(n):
            torch.distributed.barrier()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(n):
                step()
            torch.cuda.synchronize()
            torch.distributed.barrier()
            tt1 = torch.tensor([time.perf_counter() - t1], dtype=torch.float64, device=dev)
            torch.distributed.all_reduce(tt1, op=torch.distributed.ReduceOp.MAX)
            return float(tt1.item())
        for cand in ("ksharded", "sharded", "bf16", "autograd"):
            if cand == grad_sync_mode:
                continue
            current["mode"] = cand
            if os.environ.get("PV_BENCH_HANG_IN_MODE") == cand and rank == world - 1:      # (test hook: a rank that never arrives)
                time.sleep(1e6)
            try:
                opt.consolidate_sharded()                     # (collective) full tensors current before the layout changes
                sync.remove()                                 # (the trial step installs and removes hooks of its own)
                in_force = D.negotiate_grad_sync(model, opt, batch, cand, allow_demotion=True)
                sync = D.OverlappedGradSync(model)
            except SystemExit as e:
                other_modes[cand] = {"status": f"failed: {e}"}
                break                                          # no exchange works any more: nothing further can be timed
            if in_force != cand:
                other_modes[cand] = {"status": f"not available here: the trial step or the optimiser fell back to '{in_force}'"}
                continue
            try:
                for _ in range(min(5, max(2, args.warmup))):
                    step()
                sec = timed_steps(args.steps)
            except Exception as e:      # this rank alone may have failed: the others wait in a collective until the timer ends the leg
                other_modes[cand] = {"status": f"failed while stepping: {type(e).__name__}: {str(e)[:200]}"}
                watchdog.join()
                raise
            other_modes[cand] = {"status": "ok", "ms_per_step": round(sec / args.steps * 1e3, 3),
                                 "value": round(world * b * args.steps / sec, 2), "unit": "samples/s",
                                 "collectives": collectives_info(world, cand, in_force),
                                 "exchange_bytes_per_rank_and_step": exchange_bytes(cand, world, b, model)}
        current["mode"] = "consolidation after the last mode"
        opt.consolidate_sharded()
        watchdog.cancel()

    if rank == 0:
        out = dict(headline)
        out.update({
            "grad_sync_modes": modes_record(),
            "train_nmae_first_step": round(first, 6) if first is not None else None,
            "train_nmae_last_step": round(last, 6),
            "whole_step_frac_of_bf16_mfma_peak": round(value / world * (23.37e9 if t_frames == 18 else 25.27e9) / MFMA_BF16_PEAK, 4),
        })
        if args.full and not args.no_roofline and world == 1:
            if args.precision == "bf16":
                out["roofline"] = measure_step_rooflines(step, model, b, t_frames)
                if "avg_launch_ms" in out["roofline"]:
                    out["roofline"]["share_of_step"] = round(out["roofline"]["avg_launch_ms"] / ms_step, 3)
                if calibration:      # the same fractions against this device's own rates (scalars: the driver's record keeps them)
                    r = out["roofline"]
                    r["calibrated_copy_TBps"], r["calibrated_mfma_bf16_TFLOPs"] = calibration["copy_TBps"], calibration["mfma_bf16_TFLOPs"]
                    if "achieved" in r:
                        r["frac_of_calibrated_copy"] = round(r["achieved"] / 1e3 / calibration["copy_TBps"], 4)
                    r["all_conv_frac_calibrated"] = round(r["all_conv_frac"] * MFMA_BF16_PEAK / 1e12 / calibration["mfma_bf16_TFLOPs"], 4)
                    if "all_conv_hbm_frac" in r:
                        r["all_conv_hbm_frac_calibrated"] = round(r["all_conv_hbm_frac"] * HBM_PEAK / 1e12 / calibration["copy_TBps"], 4)
                    if "conv_fwd_dgrad_frac" in r:
                        r["conv_fwd_dgrad_frac_calibrated"] = round(r["conv_fwd_dgrad_frac"] * MFMA_BF16_PEAK / 1e12 / calibration["mfma_bf16_TFLOPs"], 4)
            else:
                out["roofline"] = None
            del model, opt, batch
            settle()
            if args.precision == "bf16" and out["roofline"] is not None:
                # the clock the conv kernels really run at (a wave's own counters; sysfs above averages over ~10 ms), and the conv
                # fraction against the matrix peak AT THAT CLOCK: the 2.5 PFLOP/s of the guide is a 2.4 GHz figure
                try:
                    ec = out["engine_clock_under_kernels"] = measure_engine_clocks(dev, b)
                    r = out["roofline"]
                    conv_mhz = [ec[k]["median_MHz"] for k in ("conv_forward_32_to_32", "conv_weight_gradient") if "median_MHz" in ec.get(k, {})]
                    if conv_mhz:
                        r["sclk_MHz_under_conv_kernels"] = round(sum(conv_mhz) / len(conv_mhz))
                        r["sclk_MHz_under_bare_mfma_loop"] = ec["bare_mfma_loop"].get("median_MHz")
                        r["sclk_MHz_under_fc1_pass"] = ec["fc1_one_pass_backward"].get("median_MHz")
                        r["all_conv_frac_at_running_clock"] = round(r["all_conv_frac"] * 2400.0 / r["sclk_MHz_under_conv_kernels"], 4)
                except Exception as e:      # noqa: BLE001 -- a diagnostic must not cost the line
                    out["engine_clock_under_kernels"] = {"error": f"{type(e).__name__}: {e}"}
                settle()
            if not args.no_extras:
                out["config3"] = measure_config3(dev, b, args.history_minutes)
                settle()
                if out["roofline"] is not None:      # scalars the driver's record keeps (it drops nested objects)
                    out["roofline"]["config3_pipeline_ms"] = out["config3"]["pipeline_ms"]
                    out["roofline"]["config3_frac"] = out["config3"]["frac_of_survey_roofline"]
                    out["roofline"]["config3_joined_step_ms"] = out["config3"]["joined_train_step"]["ms_per_step"]
                if args.precision == "bf16":
                    out["hip_graph_step"] = measure_graph_step(dev, b, args.history_minutes)
                    settle()
                    if args.history_minutes != 60:   # the reference default (model.py:22-23 history_minutes=60): 19 frames
                        out["t19"] = dict(measure_batch_sweep(dev, 60, batches=(b,), steps=30, warmup=8)[f"B={b}"], t_frames=19,
                                          history_minutes=60, per_gpu_batch=b)
                        out["t19"]["whole_step_frac_of_bf16_mfma_peak"] = round(out["t19"]["samples_per_s"] * 25.27e9 / MFMA_BF16_PEAK, 4)
                    out["batch_sweep"] = measure_batch_sweep(dev, args.history_minutes)
                    # the N = 1 anchor of the strong-scaling mode (--global-batch 512: what 8 GPUs split 64 samples each)
                    sb = measure_batch_sweep(dev, args.history_minutes, batches=(512,), steps=5, warmup=2)["B=512"]
                    out["strong_b512"] = dict(sb, n_gpus=1, global_batch=512,
                                              note="python bench.py --gpus 1 --global-batch 512 times the same step as the headline line")
                    out["strong_b512"]["one_rank_of_8"] = measure_sharded_rank_compute(dev, args.history_minutes)
                    r8 = out["strong_b512"]["one_rank_of_8"]
                    if "aggregate_samples_per_s_if_exchange_hides" in r8:
                        r8["ceiling_over_one_gpu"] = round(r8["aggregate_samples_per_s_if_exchange_hides"] / sb["samples_per_s"], 2)
                    # the K-sharded mix (fc1's columns dealt over the ranks): strong (64 per GPU) and weak (32 per GPU) scaling
                    k8 = out["strong_b512"]["one_rank_of_8_ksharded"] = measure_ksharded_rank_compute(dev, args.history_minutes, per_gpu_batch=64)
                    if "aggregate_samples_per_s_if_exchange_hides" in k8:
                        k8["ceiling_over_one_gpu"] = round(k8["aggregate_samples_per_s_if_exchange_hides"] / sb["samples_per_s"], 2)
                    out["weak_b32_one_rank_of_8_ksharded"] = measure_ksharded_rank_compute(dev, args.history_minutes, per_gpu_batch=b)
                    if out["roofline"] is not None:
                        out["roofline"]["batch64_samples_per_s"] = out["batch_sweep"].get("B=64", {}).get("samples_per_s")
                        out["roofline"]["one_rank_of_8_ms_at_64_per_gpu_sharded"] = r8.get("ms_per_step")
                        out["roofline"]["one_rank_of_8_ms_at_64_per_gpu_ksharded"] = k8.get("ms_per_step")
                        out["roofline"]["one_rank_of_8_ms_at_32_per_gpu_ksharded"] = out["weak_b32_one_rank_of_8_ksharded"].get("ms_per_step")
                        out["roofline"]["strong_b512_samples_per_s"] = sb["samples_per_s"]
                        out["roofline"]["strong_8gpu_ceiling_over_one_gpu"] = r8.get("ceiling_over_one_gpu")
                        out["roofline"]["strong_8gpu_ceiling_over_one_gpu_ksharded"] = k8.get("ceiling_over_one_gpu")
                    out["fp32"] = measure_fp32_headline(dev, b, args.history_minutes)
                    if out["roofline"] is not None:      # (a scalar the driver's record keeps)
                        out["roofline"]["fp32_samples_per_s"] = out["fp32"]["value"]
                    settle()
                out["other_models"] = measure_other_models(dev)
                settle()
        else:
            out["roofline"] = distributed_roofline or None
        if args.full and not args.no_cpu_baseline and world == 1:
            out["val_nmae"], out["cpu_baseline"] = matched_validation_and_cpu_baseline(dev, args.history_minutes)
            if out.get("roofline"):      # scalars the driver's record keeps
                out["roofline"]["val_nmae_bf16_minus_fp32"] = out["val_nmae"]["paired_bf16_minus_fp32"]["mean"]
                out["roofline"]["val_nmae_bf16_minus_fp32_se"] = out["val_nmae"]["paired_bf16_minus_fp32"]["standard_error"]
                out["roofline"]["val_nmae_seeds"] = out["val_nmae"]["n_seeds"]
                out["roofline"]["val_nmae_pass"] = out["val_nmae"]["pass"]
            flow_cpu = flow_cpu_baseline()
            if "config3" in out:
                out["config3"]["cpu_baseline"] = flow_cpu
                out["config3"]["speedup_vs_all_threads"] = round(out["config3"]["samples_per_s"] / flow_cpu["all_threads"]["samples_per_s"], 1)
            else:
                out["flow_cpu_baseline"] = flow_cpu
        else:
            out["cpu_baseline"] = None
        print(json.dumps(out))
    if distributed:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
