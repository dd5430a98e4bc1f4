"""Tensor-level wrappers over the C ABI (include/pv_yield_hip.h).

Every function here launches hand-written gfx950 kernels through libpvyield_hip.so on torch's current
HIP stream.  torch is used for device memory and streams only.  There is no CPU fallback: CPU tensors
or a missing library raise.
"""
import ctypes
from typing import Callable, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import (Conv3dDims, Conv3dGeom, FarnebackParams, PV_BORDER_CONSTANT, PV_BORDER_REPLICATE,
                   PV_OPTFLOW_FARNEBACK_GAUSSIAN, check, current_stream_ptr, get_lib, ptr, require_cuda)

c_i32, c_i64, c_f32, c_f64, c_sz = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_double, ctypes.c_size_t


# ------------------------------------------------------------------------------------------------
# optical-flow advection
# ------------------------------------------------------------------------------------------------
def u8_from_10bit(x: torch.Tensor, mode: int = 0, return_flag: bool = False):
    """convert_10bpp_to_uint8 (notebooks/13_...ipynb:112-119); x int16 or float32, any shape."""
    require_cuda(x)
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    flag = torch.zeros(1, dtype=torch.int32, device=x.device)
    lib = get_lib()
    if x.dtype == torch.int16:
        fn = lib.pv_u8_from_10bit_i16
    elif x.dtype == torch.float32:
        fn = lib.pv_u8_from_10bit_f32
    else:
        raise TypeError(f"u8_from_10bit: int16 or float32 expected, got {x.dtype}")
    check(fn(ptr(x), ptr(out), x.numel(), mode, ptr(flag), current_stream_ptr()), "pv_u8_from_10bit")
    return (out, flag) if return_flag else out


def make_farneback_params(pyr_scale=0.5, levels=2, winsize=40, iterations=3, poly_n=5, poly_sigma=0.7,
                          flags=PV_OPTFLOW_FARNEBACK_GAUSSIAN) -> FarnebackParams:
    return FarnebackParams(float(pyr_scale), int(levels), int(winsize), int(iterations), int(poly_n),
                           float(poly_sigma), int(flags))


_workspaces = {}
_pinned_workspaces = {}      # key -> number of live HIP graphs whose kernel arguments hold that buffer's address


def _workspace(key: str, nbytes: int, device) -> torch.Tensor:
    """Grow-only scratch buffers owned by the host side (the C ABI never allocates).  A buffer that a live HIP graph
    replays into (pin_workspaces) is never replaced: a request that outgrows it raises instead of freeing memory the graph
    still writes."""
    k = (key, str(device))
    buf = _workspaces.get(k)
    if buf is None or buf.numel() < nbytes:
        if buf is not None and _pinned_workspaces.get(k, 0) > 0:
            raise RuntimeError(
                f"workspace '{key}' ({buf.numel()} bytes) is held by a captured HIP graph (graphs.GraphedTrainStep) and a call "
                f"now needs {nbytes} bytes: replacing it would leave the graph replaying into freed memory.  Run the larger "
                f"call (e.g. a bigger validation batch, a second model) once BEFORE capturing, or release the graph "
                f"(GraphedTrainStep.close()).")
        buf = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
        _workspaces[k] = buf
    return buf


def pin_workspaces():
    """Marks every workspace that exists now as held by a captured graph; returns the token for unpin_workspaces."""
    keys = list(_workspaces)
    for k in keys:
        _pinned_workspaces[k] = _pinned_workspaces.get(k, 0) + 1
    return keys


def unpin_workspaces(keys) -> None:
    for k in keys or ():
        n = _pinned_workspaces.get(k, 0) - 1
        if n > 0:
            _pinned_workspaces[k] = n
        else:
            _pinned_workspaces.pop(k, None)


def farneback_stack(frames_u8: torch.Tensor, **kwargs) -> torch.Tensor:
    """compute_optical_flow (notebooks/13_...ipynb:175-240) for a batch of frame stacks.
    frames_u8: [..., T, H, W] uint8 -> flow [..., T-1, H, W, 2] float32, one Farnebäck field per
    consecutive pair.  One batched launch sequence replaces the reference's process pool."""
    require_cuda(frames_u8)
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() < 3:
        raise TypeError("farneback_stack: uint8 [..., T, H, W] expected")
    *lead, t, h, w = frames_u8.shape
    n_stacks = int(np.prod(lead)) if lead else 1
    if t < 2:
        raise ValueError("farneback_stack: need at least 2 frames")
    params = make_farneback_params(**kwargs)
    lib = get_lib()
    flows = torch.empty((*lead, t - 1, h, w, 2), dtype=torch.float32, device=frames_u8.device)
    if n_stacks == 0:
        return flows
    n_pairs = n_stacks * (t - 1)
    need = c_sz(0)
    check(lib.pv_farneback_workspace_bytes(n_pairs, h, w, ctypes.byref(params), ctypes.byref(need)),
          "pv_farneback_workspace_bytes")
    ws = _workspace("farneback", need.value, frames_u8.device)
    hw = h * w
    base = frames_u8.data_ptr()
    check(lib.pv_farneback_batch_u8(ctypes.c_void_p(base), ctypes.c_void_p(base + hw), hw, hw, t - 1, t * hw,
                                    ptr(flows), n_pairs, h, w, ctypes.byref(params), ptr(ws), ws.numel(),
                                    current_stream_ptr()), "pv_farneback_batch_u8")
    return flows


def farneback_pairs(prev_u8: torch.Tensor, next_u8: torch.Tensor, **kwargs) -> torch.Tensor:
    """cv.calcOpticalFlowFarneback batched: prev/next uint8 [N, H, W] -> flow f32 [N, H, W, 2]."""
    require_cuda(prev_u8, next_u8)
    if prev_u8.shape != next_u8.shape or prev_u8.dtype != torch.uint8 or next_u8.dtype != torch.uint8:
        raise TypeError("farneback_pairs: two uint8 tensors of equal shape expected")
    n, h, w = prev_u8.shape
    params = make_farneback_params(**kwargs)
    lib = get_lib()
    need = c_sz(0)
    check(lib.pv_farneback_workspace_bytes(n, h, w, ctypes.byref(params), ctypes.byref(need)),
          "pv_farneback_workspace_bytes")
    ws = _workspace("farneback", need.value, prev_u8.device)
    flow = torch.empty((n, h, w, 2), dtype=torch.float32, device=prev_u8.device)
    check(lib.pv_farneback_batch_u8(ptr(prev_u8), ptr(next_u8), h * w, h * w, 0, 0, ptr(flow), n, h, w, ctypes.byref(params),
                                    ptr(ws), ws.numel(), current_stream_ptr()), "pv_farneback_batch_u8")
    return flow


def flow_weighted_mean(flows: torch.Tensor, weights: Optional[Sequence[float]] = None) -> torch.Tensor:
    """weighted_average (notebooks/optical_flow_1.ipynb:293-294): flows [G, N, ...] -> [G, ...]."""
    require_cuda(flows)
    if flows.dtype != torch.float32 or flows.dim() < 3:
        raise TypeError("flow_weighted_mean: float32 [G, N, ...] expected")
    g, n = flows.shape[:2]
    elems = flows[0, 0].numel()
    out = torch.empty((g, *flows.shape[2:]), dtype=torch.float32, device=flows.device)
    warr = None
    if weights is not None:
        warr = (c_f64 * n)(*[float(v) for v in weights])
    check(get_lib().pv_flow_weighted_mean_f32(ptr(flows), warr, ptr(out), g, n, elems, current_stream_ptr()),
          "pv_flow_weighted_mean_f32")
    return out


def remap_bilinear(src: torch.Tensor, flow: torch.Tensor, n_steps: int = 1, step0: float = 1.0,
                   border_mode: int = PV_BORDER_CONSTANT, border_value: float = float("nan"),
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """remap_image batched (notebooks/13_...ipynb:259-281): src [N,H,W] (f32 or u8), flow f32 [N,H,W,2]
    -> dst [N, n_steps, H, W]; step s is cv.remap(src, meshgrid - flow*(step0+s), INTER_LINEAR, border)."""
    require_cuda(src, flow)
    n, h, w = src.shape
    if flow.shape != (n, h, w, 2) or flow.dtype != torch.float32:
        raise TypeError("remap_bilinear: flow must be float32 [N,H,W,2] matching src")
    if out is None:
        out = torch.empty((n, n_steps, h, w), dtype=src.dtype, device=src.device)
        img_stride, step_stride = n_steps * h * w, h * w
    else:
        require_cuda(out)
        if out.shape != (n, n_steps, h, w) or out.dtype != src.dtype:
            raise TypeError("remap_bilinear: bad out tensor")
        img_stride, step_stride = out.stride(0), out.stride(1)
    lib = get_lib()
    if src.dtype == torch.float32:
        check(lib.pv_remap_bilinear_f32(ptr(src), h * w, ptr(flow), h * w * 2, ptr(out), img_stride, step_stride, n,
                                        n_steps, step0, h, w, border_mode, border_value, current_stream_ptr()),
              "pv_remap_bilinear_f32")
    elif src.dtype == torch.uint8:
        bv = 0 if border_value != border_value else int(border_value)
        check(lib.pv_remap_bilinear_u8(ptr(src), h * w, ptr(flow), h * w * 2, ptr(out), img_stride, step_stride, n,
                                       n_steps, step0, h, w, border_mode, bv, current_stream_ptr()),
              "pv_remap_bilinear_u8")
    else:
        raise TypeError("remap_bilinear: float32 or uint8 images expected")
    return out


def remap_bilinear_strided(src_ptr: int, src_stride: int, flow: torch.Tensor, out_ptr: int, out_image_stride: int,
                           out_step_stride: int, n: int, n_steps: int, step0: float, h: int, w: int,
                           border_mode: int, border_value: float, flow_stride: Optional[int] = None) -> None:
    """f32 remap on raw strided views (used to write advected frames straight into the conv input stack).  flow_stride
    (elements between the fields of consecutive images; default one field [h, w, 2] each): 0 advects every image along
    the one field `flow` points at."""
    check(get_lib().pv_remap_bilinear_f32(ctypes.c_void_p(src_ptr), src_stride, ptr(flow),
                                          h * w * 2 if flow_stride is None else flow_stride,
                                          ctypes.c_void_p(out_ptr), out_image_stride, out_step_stride, n, n_steps,
                                          step0, h, w, border_mode, border_value, current_stream_ptr()),
          "pv_remap_bilinear_f32")


_LAYOUT_DIMS = {"NCTHW": (0, 2, 1, 3, 4), "NTHWC": (0, 1, 4, 2, 3)}      # positions of (b, t, c, rows, columns)


def _layout_dims(who: str, x: torch.Tensor, layout: str):
    if layout not in _LAYOUT_DIMS:
        raise ValueError(f"{who}: layout must be 'NCTHW' or 'NTHWC', got {layout!r}")
    if x.dtype != torch.float32 or x.dim() != 5:
        raise TypeError(f"{who}: float32 [B,C,T,H,W] (NCTHW) or [B,T,H,W,C] (NTHWC) expected, got {x.dtype} {tuple(x.shape)}")
    return _LAYOUT_DIMS[layout]


def u8_stacks_from_normalised(x: torch.Tensor, t_obs: int, counts_scale: float, layout: str = "NCTHW",
                              channel: Optional[int] = None) -> torch.Tensor:
    """Normalised f32 frames -> the u8 frame stacks farneback_stack takes, one pass (pv_u8_stacks_from_normalised_f32):
    u8 = round_half_even(clamp(x * float32(4 * counts_scale) + 512, 0, 1020) / 4) of the first t_obs time slices.
    x: [B,C,T,H,W] (layout "NCTHW") or [B,T,H,W,C] ("NTHWC"), any strides whose image rows follow each other
    (stride(rows) == W * stride(columns)); -> u8 [B, C, t_obs, H, W], or [B, 1, t_obs, H, W] for `channel` = i."""
    _require_device(x)       # a strided view is fine: the kernel reads through element strides
    db, dt, dc, dh, dw = _layout_dims("u8_stacks_from_normalised", x, layout)
    b, t, c, h, w = (x.shape[d] for d in (db, dt, dc, dh, dw))
    if not 1 <= t_obs <= t:
        raise ValueError(f"u8_stacks_from_normalised: t_obs = {t_obs} outside 1..{t}")
    if channel is not None and not 0 <= channel < c:
        raise ValueError(f"u8_stacks_from_normalised: channel {channel} outside 0..{c - 1}")
    if x.stride(dh) != w * x.stride(dw) or min(x.stride()) < 0:
        raise TypeError("u8_stacks_from_normalised: the rows of an image must follow each other in memory")
    out = torch.empty((b, c if channel is None else 1, t_obs, h, w), dtype=torch.uint8, device=x.device)
    if out.numel():
        check(get_lib().pv_u8_stacks_from_normalised_f32(ptr(x), x.stride(db), x.stride(dt), x.stride(dc), x.stride(dw),
                                                         ptr(out), b, t_obs, c, h * w, -1 if channel is None else channel,
                                                         4.0 * counts_scale, current_stream_ptr()),
              "pv_u8_stacks_from_normalised_f32")
    return out


def remap_bilinear_nhwc(src: torch.Tensor, flow: torch.Tensor, out: torch.Tensor, step0: float = 1.0,
                        border_mode: int = PV_BORDER_CONSTANT, border_value: float = float("nan")) -> torch.Tensor:
    """remap_bilinear on channels-last frames (pv_remap_bilinear_nhwc_f32): src f32 [N,H,W,C] (frame strides free, each
    frame dense), flow f32 [N,C,H,W,2] (per channel) or [N,H,W,2] (shared by the C channels), out f32 [N,n_steps,H,W,C]
    (image and step strides free) <- cv.remap(src[n,:,:,c], meshgrid - flow*(step0+s), INTER_LINEAR, border)."""
    _require_device(src, flow, out)      # src and out are time slices of one tensor: strided, each frame dense
    if src.dtype != torch.float32 or src.dim() != 4 or out.dtype != torch.float32 or out.dim() != 5:
        raise TypeError("remap_bilinear_nhwc: float32 src [N,H,W,C] and out [N,n_steps,H,W,C] expected")
    n, h, w, c = src.shape
    n_steps = out.shape[1]
    if out.shape != (n, n_steps, h, w, c) or src.stride()[1:] != (w * c, c, 1) or out.stride()[2:] != (w * c, c, 1):
        raise TypeError("remap_bilinear_nhwc: out must be [N,n_steps,H,W,C] like src; frames must be dense")
    if flow.dtype != torch.float32 or not flow.is_contiguous() or tuple(flow.shape) not in ((n, c, h, w, 2), (n, h, w, 2)):
        raise TypeError("remap_bilinear_nhwc: flow must be contiguous float32 [N,C,H,W,2] or [N,H,W,2]")
    per_channel = flow.dim() == 5
    if n and n_steps:
        check(get_lib().pv_remap_bilinear_nhwc_f32(ptr(src), src.stride(0), ptr(flow), (c if per_channel else 1) * h * w * 2,
                                                   h * w * 2 if per_channel else 0, ptr(out), out.stride(0), out.stride(1), n,
                                                   n_steps, step0, h, w, c, border_mode, border_value, current_stream_ptr()),
              "pv_remap_bilinear_nhwc_f32")
    return out


def ssim_mean(im1: torch.Tensor, im2: torch.Tensor, data_range: Optional[float] = None) -> torch.Tensor:
    """Mean structural similarity of image pairs [N, H, W] (uint8 or float32), skimage's defaults (pv_ssim_mean_*): f64 [N]."""
    require_cuda(im1, im2)
    if im1.shape != im2.shape or im1.dim() != 3 or im1.dtype != im2.dtype or im1.dtype not in (torch.uint8, torch.float32):
        raise TypeError("ssim_mean: two uint8 or two float32 tensors [N, H, W] of one shape")
    im1, im2 = im1.contiguous(), im2.contiguous()
    n, h, w = im1.shape
    if data_range is None:
        data_range = 255.0 if im1.dtype == torch.uint8 else 2.0      # scikit-image: the dtype's range
    out = torch.empty(n, dtype=torch.float64, device=im1.device)
    fn = get_lib().pv_ssim_mean_u8 if im1.dtype == torch.uint8 else get_lib().pv_ssim_mean_f32
    check(fn(ptr(im1), h * w, ptr(im2), h * w, n, h, w, float(data_range), ptr(out), current_stream_ptr()), "pv_ssim_mean")
    return out


def prepare_stacks(raw: torch.Tensor, mean: torch.Tensor, std: torch.Tensor, t_out: int, mode: int = 0):
    """raw [B,T,C,H,W] int16/f32 counts -> (u8 [B,C,T,H,W], out f32 [B,C,t_out,H,W] with slices 0..T-1 normalised).
    One pass over raw (pv_prepare_stacks_*); H*W must be a multiple of 8."""
    require_cuda(raw, mean, std)
    if raw.dtype not in (torch.int16, torch.float32) or raw.dim() != 5 or not raw.is_contiguous():
        raise TypeError("prepare_stacks: contiguous int16 or float32 [B,T,C,H,W] expected")
    b, t, c, h, w = raw.shape
    u8 = torch.empty((b, c, t, h, w), dtype=torch.uint8, device=raw.device)
    out = torch.empty((b, c, t_out, h, w), dtype=torch.float32, device=raw.device)
    lib = get_lib()
    fn = lib.pv_prepare_stacks_i16 if raw.dtype == torch.int16 else lib.pv_prepare_stacks_f32
    check(fn(ptr(raw), ptr(u8), ptr(out), b, t, c, h * w, t_out, mode, ptr(mean), ptr(std), None, current_stream_ptr()),
          "pv_prepare_stacks")
    return u8, out


def normalise(x: torch.Tensor, mean: torch.Tensor, std: torch.Tensor, inner: int,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(x - mean[c]) / std[c] with c = (flat_index // inner) % len(mean); x int16 or f32."""
    require_cuda(x, mean, std)
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    lib = get_lib()
    fn = lib.pv_normalise_i16 if x.dtype == torch.int16 else lib.pv_normalise_f32
    if x.dtype not in (torch.int16, torch.float32):
        raise TypeError("normalise: int16 or float32 expected")
    check(fn(ptr(x), ptr(out), x.numel(), inner, mean.numel(), ptr(mean), ptr(std), current_stream_ptr()),
          "pv_normalise")
    return out


# ------------------------------------------------------------------------------------------------
# Conv3D
# ------------------------------------------------------------------------------------------------
def conv_dims(batch, c_in, c_out, t, h, w, padding=(0, 0, 0)) -> Conv3dDims:
    return Conv3dDims(batch, c_in, c_out, t, h, w, padding[0], padding[1], padding[2])


def bf16_cpad(c: int) -> int:
    v = get_lib().pv_bf16_cpad(c)
    if v <= 0:
        raise ValueError(f"bf16 path supports 1..32 channels, got {c}")
    return v


def pack_ncdhw_f32_to_ndhwc_bf16(x: torch.Tensor) -> torch.Tensor:
    require_cuda(x)
    b, c, t, h, w = x.shape
    xp = torch.empty((b, t, h, w, bf16_cpad(c)), dtype=torch.bfloat16, device=x.device)
    check(get_lib().pv_pack_ncdhw_f32_to_ndhwc_bf16(ptr(x), ptr(xp), b, c, t, h, w, current_stream_ptr()),
          "pv_pack_ncdhw_f32_to_ndhwc_bf16")
    return xp


def pack_split2_ncdhw_f32_to_ndhwc_f16(x: torch.Tensor, maxabs_state: Optional[torch.Tensor] = None, cpad32: bool = False):
    """x f32 [B,C,T,H,W] -> (h, l, state): two half-float [B,T,H,W,CPAD] images with x s = h + l (22 significant bits) and
    state = device f32[3] (scratch, s, 1/s), s the power of two that brings max |x| below 2^14.  T*H*W must be a multiple of 4.
    maxabs_state: the state relu_gate_f32(..., want_max=True) produced together with x (its word 0 holds the bits of max |x|):
    the pass that finds the maximum is skipped.  cpad32: images of 32 channels whatever C (conv3d_f32_on_f16x2's operands)."""
    require_cuda(x)
    if x.dtype != torch.float32 or x.dim() != 5 or not x.is_contiguous():
        raise TypeError("pack_split2_ncdhw_f32_to_ndhwc_f16: a contiguous float32 [B,C,T,H,W] tensor is expected")
    b, c, t, h, w = x.shape
    planes = torch.empty((2, b, t, h, w, 32 if cpad32 else bf16_cpad(c)), dtype=torch.float16, device=x.device)
    state = maxabs_state
    have_max = state is not None
    if not have_max:
        state = torch.empty(3, dtype=torch.float32, device=x.device)
    check(get_lib().pv_pack_split2_ncdhw_f32_to_ndhwc_f16(ptr(x), ptr(planes[0]), ptr(planes[1]), ptr(state), int(have_max) | (2 if cpad32 else 0), b, c, t,
                                                          h, w, current_stream_ptr()), "pv_pack_split2_ncdhw_f32_to_ndhwc_f16")
    return planes[0], planes[1], state


def conv3d_bwd_weight_f16(x: torch.Tensor, dy: torch.Tensor, c_in: int, c_out: int, padding=(0, 0, 0), out=None):
    """conv3d_bwd_weight_bf16 on half-float operand images: x [B,T,H,W,CPAD] f16, dy [B,To,Ho,Wo,32] f16.
    out: (dw, db) contiguous f32 tensors of c_out * c_in * 27 / c_out elements to write into (else fresh ones)."""
    require_cuda(x, dy)
    b, t, h, w, cpad = x.shape
    d = conv_dims(b, c_in, c_out, t, h, w, padding)
    need = c_sz(0)
    lib = get_lib()
    check(lib.pv_conv3d_bwd_weight_bf16_workspace_bytes(ctypes.byref(d), ctypes.byref(need)), "wgrad workspace")
    ws = _workspace("wgrad", need.value, x.device)
    if out is None:
        dw = torch.empty((c_out, c_in, 3, 3, 3), dtype=torch.float32, device=x.device)
        db = torch.empty(c_out, dtype=torch.float32, device=x.device)
    else:
        dw, db = out
        if dw.numel() != c_out * c_in * 27 or db.numel() != c_out or not (dw.is_contiguous() and db.is_contiguous()):
            raise ValueError("conv3d_bwd_weight_f16: out = (dw, db) must be contiguous f32 tensors of the gradients' sizes")
    check(lib.pv_conv3d_bwd_weight_f16(ptr(x), ptr(dy), ptr(dw), ptr(db), ctypes.byref(d), ptr(ws), ws.numel(),
                                       current_stream_ptr()), "pv_conv3d_bwd_weight_f16")
    return dw, db


def conv3d_bwd_weight_f32_on_f16x2(x: torch.Tensor, dy: torch.Tensor, padding=(0, 0, 0), dy_maxabs_state=None):
    """Weight and bias gradient of a 3x3x3, stride-1 Conv3d with 32 output channels at f32 accuracy on the F16 matrix cores:
    x f32 [B,Ci<=32,T,H,W] and dy f32 [B,32,To,Ho,Wo] (already multiplied by the ReLU derivative) are each scaled by a power of
    two and split in two half-float terms (22 bits), the weight-gradient kernel runs on the three operand pairs whose product
    is above 2^-22 of the result -- (l,h), (h,l), (h,h) -- and the three f32 results are added in that order, then un-scaled.
    (Round 3's three-term bf16 split -- six launches, 10 bytes of split traffic per element -- was removed in round 6.)
    -> (dw [32,Ci,3,3,3], db [32])."""
    ci = x.shape[1]
    xh, xl, xs = pack_split2_ncdhw_f32_to_ndhwc_f16(x)
    dh, dl, ds = pack_split2_ncdhw_f32_to_ndhwc_f16(dy, maxabs_state=dy_maxabs_state)
    parts = torch.empty((3, 32 * ci * 27), dtype=torch.float32, device=x.device)
    dbp = torch.empty((2, 32), dtype=torch.float32, device=x.device)
    for i, (px, pd) in enumerate(((xl, dh), (xh, dl), (xh, dh))):
        dw_i, db_i = conv3d_bwd_weight_f16(px, pd, ci, 32, padding)
        parts[i].copy_(dw_i.reshape(-1))
        if i >= 1:
            dbp[i - 1].copy_(db_i)       # the bias gradient is the plain sum of dy: one term per plane of dy (l, then h)
    dw = torch.empty((32, ci, 3, 3, 3), dtype=torch.float32, device=x.device)
    check(get_lib().pv_sum_slabs_acc_f32(ptr(parts), ptr(dw), parts.shape[1], 3, 0, current_stream_ptr()), "pv_sum_slabs_acc_f32")
    db = torch.empty(32, dtype=torch.float32, device=x.device)
    check(get_lib().pv_sum_slabs_acc_f32(ptr(dbp), ptr(db), 32, 2, 0, current_stream_ptr()), "pv_sum_slabs_acc_f32")
    dw.mul_(xs[2]).mul_(ds[2])      # exact: powers of two (device scalars: no host round trip)
    db.mul_(ds[2])
    return dw, db


def conv3d_bwd_weight_f32_from_split2(xh, xl, xs, dh, dl, ds, c_in: int, padding=(0, 0, 0)):
    """conv3d_bwd_weight_f32_on_f16x2 on operand images that already exist (the f16x2 forward made x's, the f16x2 data gradient
    made dy's): three launches, no split pass.  -> (dw [32,c_in,3,3,3], db [32])."""
    parts = torch.empty((3, 32 * c_in * 27), dtype=torch.float32, device=xh.device)
    dbp = torch.empty((3, 32), dtype=torch.float32, device=xh.device)      # (row 0: the bias sum of dy's l image against x_l: not a term)
    for i, (px, pd) in enumerate(((xl, dh), (xh, dl), (xh, dh))):
        conv3d_bwd_weight_f16(px, pd, c_in, 32, padding, out=(parts[i], dbp[(i + 2) % 3]))      # db: (dh, dl, dh) -> rows 2, 0, 1: rows 0, 1 = l, h
    dw = torch.empty((32, c_in, 3, 3, 3), dtype=torch.float32, device=xh.device)
    check(get_lib().pv_sum_slabs_acc_f32(ptr(parts), ptr(dw), parts.shape[1], 3, 0, current_stream_ptr()), "pv_sum_slabs_acc_f32")
    db = torch.empty(32, dtype=torch.float32, device=xh.device)
    check(get_lib().pv_sum_slabs_acc_f32(ptr(dbp), ptr(db), 32, 2, 0, current_stream_ptr()), "pv_sum_slabs_acc_f32")
    dw.mul_(xs[2] * ds[2])      # exact: powers of two (device scalars: no host round trip)
    db.mul_(ds[2])
    return dw, db


def conv3d_pack_weight_split2_f16(w: torch.Tensor):
    """w f32 [c_out<=32, c_in<=32, 3,3,3] -> (wp f16 [4, elems]: forward operator (h, l), data-gradient operator (h, l); state f32[3])."""
    require_cuda(w)
    if w.dtype != torch.float32 or w.dim() != 5 or tuple(w.shape[2:]) != (3, 3, 3) or not w.is_contiguous():
        raise TypeError("conv3d_pack_weight_split2_f16: a contiguous float32 [Co,Ci,3,3,3] weight is expected")
    lib = get_lib()
    n = int(lib.pv_conv3d_split2_weight_elems())
    wp = torch.empty((4, n // 4), dtype=torch.float16, device=w.device)
    state = torch.empty(69, dtype=torch.float32, device=w.device)      # (max bits, s, 1 / s, -, -, 32 + 32 absolute row sums)
    check(lib.pv_conv3d_pack_weight_split2_f16(ptr(w), ptr(wp), ptr(state), w.shape[0], w.shape[1], current_stream_ptr()),
          "pv_conv3d_pack_weight_split2_f16")
    return wp, state


F16X2_SMALL_PRODUCTS_F16 = True      # conv3d_f32_on_f16x2: x_l w_h and x_h w_l leave the matrix cores as half floats (False: f32, the cross-check)


def conv3d_f16x2_covers(batch, c_in, c_out, t, h, w, padding) -> bool:
    """Does the f16x2 form (conv3d_f32_on_f16x2) take this layer?  (64-byte voxels, >= 2 output slices per time chunk, size limits)"""
    d = conv_dims(batch, c_in, c_out, t, h, w, padding)
    return bool(get_lib().pv_conv3d_fwd_f16_f32out_covers(ctypes.byref(d)))


def conv3d_f32_on_f16x2(xh, xl, xs, wp_h, wp_l, ws, c_in: int, c_out: int, padding=(0, 0, 0), bias=None, relu=False, gate_h=None,
                        data_gradient=False, want_planes=True, want_f32=True):
    """One f32 Conv3d (3x3x3, stride 1, 32 output channels of the OPERATOR) from split operand images: xh / xl f16 [B,T,H,W,32]
    with scale state xs, wp_h / wp_l ONE operator's fragments with state ws (data_gradient: the transposed-flipped operator's).
    Three matrix-core launches into partial tensors, then one pass: ordered sum, un-scale, bias, ReLU / gate (gate_h: the h image
    [B,To,Ho,Wo,32] of the gating activation), NCDHW -- and, want_planes, y's own split for the next layer.
    want_f32=False: only the split is written (a consumer that reads operand images).
    -> (y f32 [B,32,To,Ho,Wo] or None, state f32[3] = (bits of max |y|, s_y, 1 / s_y), planes f16 [2,B,To,Ho,Wo,32] or None)."""
    if not (want_planes or want_f32):
        raise ValueError("conv3d_f32_on_f16x2: nothing to write")
    require_cuda(xh, xl)
    b, t, h, w, cpad = xh.shape
    if cpad != 32:
        raise ValueError("conv3d_f32_on_f16x2: 64-byte voxels (17..32 input channels) are expected")
    d = conv_dims(b, c_in, c_out, t, h, w, padding)
    to, ho, wo = t + 2 * padding[0] - 2, h + 2 * padding[1] - 2, w + 2 * padding[2] - 2
    lib = get_lib()
    st = current_stream_ptr()
    if F16X2_SMALL_PRODUCTS_F16:      # the two small products as half floats (2^-12 of the accumulators): half their bytes
        p01 = torch.empty((2, b, to, ho, wo, 32), dtype=torch.float16, device=xh.device)
        parts = torch.empty((1, b, to, ho, wo, 32), dtype=torch.float32, device=xh.device)
        outs = ((p01[0], 1), (p01[1], 1), (parts[0], 0))
    else:
        p01 = None
        parts = torch.empty((3, b, to, ho, wo, 32), dtype=torch.float32, device=xh.device)
        outs = ((parts[0], 0), (parts[1], 0), (parts[2], 0))
    for (px, pw), (out, is16) in zip(((xl, wp_h), (xh, wp_l), (xh, wp_h)), outs):
        check(lib.pv_conv3d_fwd_f16_f32out(ptr(px), ptr(pw), ptr(out), is16, ctypes.byref(d), st), "pv_conv3d_fwd_f16_f32out")
    y = torch.empty((b, 32, to, ho, wo), dtype=torch.float32, device=xh.device) if want_f32 else None
    state = torch.zeros(3, dtype=torch.float32, device=xh.device)
    planes = torch.empty((2, b, to, ho, wo, 32), dtype=torch.float16, device=xh.device) if want_planes else None
    check(lib.pv_sum3_ndhwc_to_ncdhw_f32(ptr(parts), ptr(p01), ptr(xs), ptr(ws), int(bool(data_gradient)), ptr(bias), ptr(gate_h),
                                         ptr(y), ptr(planes[0]) if want_planes else None, ptr(planes[1]) if want_planes else None,
                                         ptr(state), int(bool(relu)), b, to * ho * wo, st), "pv_sum3_ndhwc_to_ncdhw_f32")
    return y, state, planes


def unpack_ndhwc_bf16_to_ncdhw_f32(xp: torch.Tensor, c: int) -> torch.Tensor:
    require_cuda(xp)
    b, t, h, w, cpad = xp.shape
    x = torch.empty((b, c, t, h, w), dtype=torch.float32, device=xp.device)
    check(get_lib().pv_unpack_ndhwc_bf16_to_ncdhw_f32(ptr(xp), ptr(x), b, c, t, h, w, current_stream_ptr()),
          "pv_unpack_ndhwc_bf16_to_ncdhw_f32")
    return x


def repack_gate_ncdhw_to_ndhwc_bf16(dy: torch.Tensor, y_mask: Optional[torch.Tensor]) -> torch.Tensor:
    require_cuda(dy, y_mask)
    b, c, t, h, w = dy.shape
    out = torch.empty((b, t, h, w, 32), dtype=torch.bfloat16, device=dy.device)
    check(get_lib().pv_repack_gate_ncdhw_to_ndhwc_bf16(ptr(dy), ptr(y_mask), ptr(out), b, c, t, h, w,
                                                       current_stream_ptr()), "pv_repack_gate_ncdhw_to_ndhwc_bf16")
    return out


def conv3d_pack_weight_bf16(weight: torch.Tensor, transpose_flip: bool = False) -> torch.Tensor:
    require_cuda(weight)
    co, ci = weight.shape[:2]
    kch = co if transpose_flip else ci
    n = get_lib().pv_conv3d_packed_weight_elems(kch)
    wp = torch.empty(n, dtype=torch.bfloat16, device=weight.device)
    check(get_lib().pv_conv3d_pack_weight_bf16(ptr(weight), ptr(wp), co, ci, int(transpose_flip), current_stream_ptr()),
          "pv_conv3d_pack_weight_bf16")
    return wp


class stage_timing:
    """Context manager around pv_stage_timing_begin / _end: per-stage device milliseconds of the multi-kernel entry points
    (Farnebäck pyramid, advection stages) recorded with HIP events on the launching stream.
        with K.stage_timing() as st: ...pv calls...
        st.stages  ->  {label: (total_ms, occurrences)} in first-seen order"""

    def __init__(self, capacity: int = 64):
        self.capacity, self.stages = capacity, {}

    def __enter__(self):
        check(get_lib().pv_stage_timing_begin(), "pv_stage_timing_begin")
        return self

    def __exit__(self, *exc):
        names = (ctypes.c_char_p * self.capacity)()
        ms = (ctypes.c_float * self.capacity)()
        counts = (ctypes.c_int32 * self.capacity)()
        n = ctypes.c_int32(0)
        check(get_lib().pv_stage_timing_end(names, ms, counts, self.capacity, ctypes.byref(n)), "pv_stage_timing_end")
        self.stages = {names[i].decode(): (float(ms[i]), int(counts[i])) for i in range(n.value)}
        return False


def device_calibration(copy_floats: int = 128 * 1003520, mfma_iters: int = 20000, reps: int = 5) -> dict:
    """What THIS device sustains, measured with HIP events on the current stream (pv_calibrate_*): a plain device copy of
    `copy_floats` floats (default: the size of fc1's weight) and a bare bf16 matrix-instruction loop on every SIMD."""
    dev = torch.device("cuda", torch.cuda.current_device())
    a = torch.empty(copy_floats, dtype=torch.float32, device=dev).normal_()
    b = torch.empty_like(a)
    wgs = 256 * 2                                   # two 4-wave workgroups per CU: two waves per SIMD
    sink = torch.zeros(wgs, dtype=torch.float32, device=dev)
    lib = get_lib()

    def timed(fn, n):
        for _ in range(2):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n * 1e-3       # seconds per call

    t_copy = timed(lambda: check(lib.pv_calibrate_copy_f32(ptr(a), ptr(b), copy_floats, current_stream_ptr()), "pv_calibrate_copy_f32"), reps * 2)
    t_mfma = timed(lambda: check(lib.pv_calibrate_mfma_bf16(ptr(sink), wgs, mfma_iters, current_stream_ptr()), "pv_calibrate_mfma_bf16"), reps)
    flops = wgs * 4 * mfma_iters * 8 * 16384.0
    # hand the gigabyte back to the driver: left in torch's cache it changed where the NEXT allocations of the caller land, and a
    # bench leg that times individual launches read its first (HBM-bound) kernel at 160-200 us instead of 75 (round 6)
    del a, b, sink
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return {"copy_TBps": round(8.0 * copy_floats / t_copy / 1e12, 3), "copy_bytes": 8 * copy_floats,
            "mfma_bf16_TFLOPs": round(flops / t_mfma / 1e12, 1), "mfma_ms": round(t_mfma * 1e3, 3),
            "what": "pv_calibrate_copy_f32 (16 B per lane, read + write bytes) and pv_calibrate_mfma_bf16 (v_mfma_f32_16x16x32_bf16 "
                    "back to back on register operands, two waves per SIMD, non-trivial data), HIP events, this process, this device"}


def relu_mask_shape(b: int, t: int, h: int, w: int):
    """Shape of the 1-bit relu mask of an NDHWC activation [b, t, h, w, 32]: int32 [b, t, hp, wp], the plane padded to
    whole 8 x 32 tiles (pv_relu_mask_dims)."""
    hp, wp = ctypes.c_int32(), ctypes.c_int32()
    check(get_lib().pv_relu_mask_dims(h, w, ctypes.byref(hp), ctypes.byref(wp)), "pv_relu_mask_dims")
    return (b, t, hp.value, wp.value)


def conv3d_fwd_bf16(x: torch.Tensor, gate: Optional[torch.Tensor], wp: torch.Tensor, bias: Optional[torch.Tensor],
                    c_in: int, c_out: int, padding=(0, 0, 0), relu=True, y_ncdhw=False,
                    out_gate: Optional[torch.Tensor] = None, out_gate_mask: Optional[torch.Tensor] = None,
                    want_relu_mask: bool = False):
    """x [B,T,H,W,CPAD(c_in)] bf16 -> y [B,To,Ho,Wo,32] bf16 (or [B,c_out,To,Ho,Wo] if y_ncdhw).
    want_relu_mask: also return the 1-bit relu mask of y, int32 relu_mask_shape(B,To,Ho,Wo) (bit c = y[..., c] > 0):
    (y, mask).
    out_gate_mask: such a mask of `out_gate` (the dgrad epilogue then reads 4 instead of 64 bytes per voxel)."""
    require_cuda(x, gate, wp, bias, out_gate, out_gate_mask)
    b, t, h, w, cpad = x.shape
    if cpad != bf16_cpad(c_in) or x.dtype != torch.bfloat16:
        raise TypeError("conv3d_fwd_bf16: x must be bf16 [B,T,H,W,CPAD(c_in)]")
    d = conv_dims(b, c_in, c_out, t, h, w, padding)
    to, ho, wo = d.out_shape()
    shape = (b, c_out, to, ho, wo) if y_ncdhw else (b, to, ho, wo, 32)
    y = torch.empty(shape, dtype=torch.bfloat16, device=x.device)
    if out_gate is not None and tuple(out_gate.shape) != shape:
        raise TypeError("conv3d_fwd_bf16: out_gate must have the output's NDHWC shape")
    if out_gate_mask is not None and (out_gate is None or out_gate_mask.dtype != torch.int32
                                      or tuple(out_gate_mask.shape) != relu_mask_shape(*shape[:4])
                                      or not out_gate_mask.is_contiguous()):
        raise TypeError("conv3d_fwd_bf16: out_gate_mask must be the contiguous int32 relu mask of out_gate (relu_mask_shape)")
    mask = torch.empty(relu_mask_shape(*shape[:4]), dtype=torch.int32, device=x.device) if want_relu_mask else None
    check(get_lib().pv_conv3d_fwd_bf16(ptr(x), ptr(gate), ptr(wp), ptr(bias), ptr(y), ptr(out_gate), ptr(out_gate_mask),
                                       ptr(mask), ctypes.byref(d), int(relu), int(y_ncdhw), current_stream_ptr()),
          "pv_conv3d_fwd_bf16")
    return (y, mask) if want_relu_mask else y


def conv3d_fwd_bf16_f32in(x: torch.Tensor, wp: torch.Tensor, bias: Optional[torch.Tensor], c_out: int, padding=(0, 0, 0),
                          relu=True, want_packed=True, want_relu_mask=False):
    """First layer: x f32 NCDHW [B,C<=16,T,H,W] -> (y bf16 NDHWC [B,To,Ho,Wo,32], xp bf16 NDHWC [B,T,H,W,16] or None
    [, relu mask of y int32 [B,To,Ho,Wo] when want_relu_mask]).
    One pass over the input instead of pack + conv; xp is what conv3d_bwd_weight_bf16 reads."""
    require_cuda(x, wp, bias)
    if x.dtype != torch.float32 or x.dim() != 5 or not x.is_contiguous():
        raise TypeError("conv3d_fwd_bf16_f32in: x must be a contiguous f32 [B,C,T,H,W] tensor")
    b, c_in, t, h, w = x.shape
    if bf16_cpad(c_in) != 16:
        raise TypeError("conv3d_fwd_bf16_f32in: built for c_in <= 16")
    d = conv_dims(b, c_in, c_out, t, h, w, padding)
    to, ho, wo = d.out_shape()
    y = torch.empty((b, to, ho, wo, 32), dtype=torch.bfloat16, device=x.device)
    xp = torch.empty((b, t, h, w, 16), dtype=torch.bfloat16, device=x.device) if want_packed else None
    mask = torch.empty(relu_mask_shape(b, to, ho, wo), dtype=torch.int32, device=x.device) if want_relu_mask else None
    check(get_lib().pv_conv3d_fwd_bf16_f32in(ptr(x), ptr(xp), ptr(wp), ptr(bias), ptr(y), ptr(mask), ctypes.byref(d),
                                             int(relu), current_stream_ptr()), "pv_conv3d_fwd_bf16_f32in")
    return (y, xp, mask) if want_relu_mask else (y, xp)


def conv3d_bwd_weight_bf16(x: torch.Tensor, dy: torch.Tensor, y_mask: Optional[torch.Tensor], c_in: int, c_out: int,
                           padding=(0, 0, 0)):
    """x [B,T,H,W,CPAD] bf16, dy/y_mask [B,To,Ho,Wo,32] bf16 -> (dw f32 [c_out,c_in,3,3,3], db f32 [c_out])."""
    require_cuda(x, dy, y_mask)
    b, t, h, w, cpad = x.shape
    d = conv_dims(b, c_in, c_out, t, h, w, padding)
    need = c_sz(0)
    lib = get_lib()
    check(lib.pv_conv3d_bwd_weight_bf16_workspace_bytes(ctypes.byref(d), ctypes.byref(need)), "wgrad workspace")
    ws = _workspace("wgrad", need.value, x.device)
    dw = torch.empty((c_out, c_in, 3, 3, 3), dtype=torch.float32, device=x.device)
    db = torch.empty(c_out, dtype=torch.float32, device=x.device)
    check(lib.pv_conv3d_bwd_weight_bf16(ptr(x), ptr(dy), ptr(y_mask), ptr(dw), ptr(db), ctypes.byref(d), ptr(ws),
                                        ws.numel(), current_stream_ptr()), "pv_conv3d_bwd_weight_bf16")
    return dw, db


# ------------------------------------------------------------------------------------------------
# fully connected head, losses, Adam
# ------------------------------------------------------------------------------------------------
def linear_fwd_f32(x, weight, bias, relu=False):
    require_cuda(x, weight, bias)
    m, k = x.shape
    n = weight.shape[0]
    need = c_sz(0)
    lib = get_lib()
    check(lib.pv_linear_workspace_bytes(m, n, k, ctypes.byref(need)), "pv_linear_workspace_bytes")
    ws = _workspace("linear", need.value, x.device)
    y = torch.empty((m, n), dtype=torch.float32, device=x.device)
    check(lib.pv_linear_fwd_f32(ptr(x), ptr(weight), ptr(bias), ptr(y), m, n, k, int(relu), ptr(ws), ws.numel(),
                                current_stream_ptr()), "pv_linear_fwd_f32")
    return y


LINEAR_F32_SKINNY = True      # fc1-sized f32 Linears (<= 32 rows, <= 128 outputs): forward / dx as streams over the weight (False: the split-product GEMM)


def linear_f32_skinny_covers(m: int, n: int, k: int) -> bool:
    return LINEAR_F32_SKINNY and bool(get_lib().pv_linear_f32_skinny_covers(m, n, k))


def linear_fwd_f32_skinny(x, weight, bias, relu=False):
    """y = relu?(x w^T + bias), f32, exact products: x [m <= 32, k], w [n <= 128, k] (linear_f32_skinny.hip)."""
    require_cuda(x, weight, bias)
    m, k = x.shape
    n = weight.shape[0]
    lib = get_lib()
    ws = _workspace("linear_skinny", int(lib.pv_linear_fwd_f32_skinny_workspace_bytes(n)), x.device)
    y = torch.empty((m, n), dtype=torch.float32, device=x.device)
    check(lib.pv_linear_fwd_f32_skinny(ptr(x), ptr(weight), ptr(bias), ptr(y), m, n, k, int(relu), ptr(ws), ws.numel(),
                                       current_stream_ptr()), "pv_linear_fwd_f32_skinny")
    return y


def linear_dx_f32_skinny(g, weight):
    """dx = g w, f32, exact products: g [m <= 32, n <= 128], w [n, k]."""
    require_cuda(g, weight)
    m, n = g.shape
    k = weight.shape[1]
    dx = torch.empty((m, k), dtype=torch.float32, device=g.device)
    check(get_lib().pv_linear_dx_f32_skinny(ptr(g), ptr(weight), ptr(dx), m, n, k, current_stream_ptr()), "pv_linear_dx_f32_skinny")
    return dx


def linear_bwd_f32(x, weight, dy, y_mask, need_dx=True):
    require_cuda(x, weight, dy, y_mask)
    m, k = x.shape
    n = weight.shape[0]
    dx = torch.empty((m, k), dtype=torch.float32, device=x.device) if need_dx else None
    dw = torch.empty((n, k), dtype=torch.float32, device=x.device)
    db = torch.empty(n, dtype=torch.float32, device=x.device)
    check(get_lib().pv_linear_bwd_f32(ptr(x), ptr(weight), ptr(dy), ptr(y_mask), ptr(dx), ptr(dw), ptr(db), m, n, k,
                                      current_stream_ptr()), "pv_linear_bwd_f32")
    return dx, dw, db


LINEAR_FWD_MAX_ROWS = 1024     # pv_linear_fwd_bf16: rows of x per call


def linear_fwd_bf16(x_bf16, w_bf16, bias, relu=False):
    require_cuda(x_bf16, w_bf16, bias)
    m, k = x_bf16.shape
    n = w_bf16.shape[0]
    need = c_sz(0)
    lib = get_lib()
    # rows per call: 1024 for the fc1 shapes (the LDS-staged kernel walks them 64 at a time, one stream over the weights each, and
    # one reduce per call), 128 for the others (the register-tiled kernel's four row tiles)
    cap = LINEAR_FWD_MAX_ROWS if (32 <= n <= 128 and n % 16 == 0) else 128
    check(lib.pv_linear_bf16_workspace_bytes(min(m, cap), n, k, ctypes.byref(need)), "pv_linear_bf16_workspace_bytes")
    ws = _workspace("linear_bf16", need.value, x_bf16.device)
    y = torch.empty((m, n), dtype=torch.float32, device=x_bf16.device)
    for r0 in range(0, m, cap):
        rows = min(cap, m - r0)
        check(lib.pv_linear_fwd_bf16(ptr(x_bf16[r0:r0 + rows]), ptr(w_bf16), ptr(bias), ptr(y[r0:r0 + rows]), rows, n, k, int(relu),
                                     ptr(ws), ws.numel(), current_stream_ptr()), "pv_linear_fwd_bf16")
    return y


def linear_bwd_bf16(x_bf16, w_bf16, dy, y_mask, need_dx=True, need_dw=True, gate_dx_by_x=False, need_db=True):
    """gate_dx_by_x: x is a ReLU output; dx leaves multiplied by (x > 0) (the producer's ReLU derivative)."""
    require_cuda(x_bf16, w_bf16, dy, y_mask)
    m, k = x_bf16.shape
    n = w_bf16.shape[0]
    dx = torch.empty((m, k), dtype=torch.bfloat16, device=dy.device) if need_dx else None
    dw = torch.empty((n, k), dtype=torch.float32, device=dy.device) if need_dw else None
    db = torch.empty(n, dtype=torch.float32, device=dy.device) if need_db else None
    check(get_lib().pv_linear_bwd_bf16(ptr(x_bf16), ptr(w_bf16), ptr(dy), ptr(y_mask), ptr(dx), ptr(dw), ptr(db), m, n,
                                       k, int(bool(gate_dx_by_x and need_dx)), current_stream_ptr()), "pv_linear_bwd_bf16")
    return dx, dw, db


def forecast_losses(y_hat: torch.Tensor, y: torch.Tensor, need_grad: bool = True, grad_scale: float = 1.0,
                    per_horizon: bool = False):
    """(mse, nmae, mse_exp, mae_exp) as a device f32[4] and d nmae / d y_hat (base_model.py:98-103).
    y may be any strided 2-D view (e.g. batch.pv.pv_yield[:, -forecast_len:, 0]).
    per_horizon=True additionally returns f32[2, forecast_len] = (mse, mae) per forecast step (base_model.py:121-141),
    computed by the same launch."""
    require_cuda(y_hat)
    if not y.is_cuda or y.dtype != torch.float32 or y.dim() != 2 or y.shape != y_hat.shape:
        raise TypeError("forecast_losses: y must be a float32 CUDA [B, forecast_len] view matching y_hat")
    m, n = y_hat.shape
    out4 = torch.empty(4, dtype=torch.float32, device=y_hat.device)
    grad = torch.empty_like(y_hat) if need_grad else None
    horizons = torch.empty((2, n), dtype=torch.float32, device=y_hat.device) if per_horizon else None
    check(get_lib().pv_forecast_losses_f32(ptr(y_hat), ctypes.c_void_p(y.data_ptr()), y.stride(0), y.stride(1), m, n,
                                           grad_scale, ptr(out4), ptr(grad), ptr(horizons), current_stream_ptr()),
          "pv_forecast_losses_f32")
    return (out4, grad, horizons) if per_horizon else (out4, grad)


def adam_step(param, grad, exp_avg, exp_avg_sq, step: int, lr=5e-4, betas=(0.9, 0.999), eps=1e-8,
              bf16_shadow=None, grad_scale=1.0):
    require_cuda(param, grad, exp_avg, exp_avg_sq, bf16_shadow)
    check(get_lib().pv_adam_step_f32(ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), ptr(bf16_shadow),
                                     param.numel(), lr, betas[0], betas[1], eps, step, grad_scale,
                                     current_stream_ptr()), "pv_adam_step_f32")


def adam_step_multi(items, step: int, lr=5e-4, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0):
    """items: list of (param, grad, exp_avg, exp_avg_sq, bf16_shadow | None) sharing hyper-parameters and step count;
    one launch per _lib.PV_ADAM_MAX_TENSORS tensors instead of one per tensor."""
    lib = get_lib()
    for i in range(0, len(items), _lib.PV_ADAM_MAX_TENSORS):
        chunk = items[i:i + _lib.PV_ADAM_MAX_TENSORS]
        arr = (_lib.AdamTensor * len(chunk))()
        for j, (p, g, m, v, sh) in enumerate(chunk):
            require_cuda(p, g, m, v, sh)
            arr[j] = _lib.AdamTensor(ptr(p), ptr(g), ptr(m), ptr(v), ptr(sh), p.numel())
        check(lib.pv_adam_step_multi_f32(arr, len(chunk), lr, betas[0], betas[1], eps, step, grad_scale,
                                         current_stream_ptr()), "pv_adam_step_multi_f32")


def adam_scalars_advance(scalars: torch.Tensor, step: torch.Tensor, lr=5e-4, betas=(0.9, 0.999), eps=1e-8) -> None:
    """step (int32 [1], device) += 1 and scalars (float32 [>= 6], device) = the Adam scalars of that step: what the `_dev`
    forms of the Adam kernels read, so that a captured HIP graph can replay the optimiser step."""
    require_cuda(scalars, step)
    if scalars.dtype != torch.float32 or scalars.numel() < 6 or step.dtype != torch.int32:
        raise TypeError("adam_scalars_advance: float32 [6] scalars and an int32 step on the device")
    check(get_lib().pv_adam_scalars_advance(ptr(scalars), ptr(step), lr, betas[0], betas[1], eps, current_stream_ptr()),
          "pv_adam_scalars_advance")


def adam_step_multi_dev(items, scalars: torch.Tensor, grad_scale=1.0):
    """adam_step_multi with the step's scalars taken from device memory (adam_scalars_advance)."""
    lib = get_lib()
    require_cuda(scalars)
    for i in range(0, len(items), _lib.PV_ADAM_MAX_TENSORS):
        chunk = items[i:i + _lib.PV_ADAM_MAX_TENSORS]
        arr = (_lib.AdamTensor * len(chunk))()
        for j, (p, g, m, v, sh) in enumerate(chunk):
            require_cuda(p, g, m, v, sh)
            arr[j] = _lib.AdamTensor(ptr(p), ptr(g), ptr(m), ptr(v), ptr(sh), p.numel())
        check(lib.pv_adam_step_multi_dev_f32(arr, len(chunk), ptr(scalars), grad_scale, current_stream_ptr()),
              "pv_adam_step_multi_dev_f32")


def conv3d_pack_weights_multi(jobs):
    """jobs: list of (weight f32 [Co,Ci,3,3,3], packed bf16 buffer, transpose_flip); one launch for all of them."""
    lib = get_lib()
    for i in range(0, len(jobs), _lib.PV_PACK_MAX_JOBS):
        chunk = jobs[i:i + _lib.PV_PACK_MAX_JOBS]
        arr = (_lib.PackJob * len(chunk))()
        for j, (w, wp, flip) in enumerate(chunk):
            require_cuda(w, wp)
            arr[j] = _lib.PackJob(ptr(w), ptr(wp), w.shape[0], w.shape[1], int(flip))
        check(lib.pv_conv3d_pack_weights_multi_bf16(arr, len(chunk), current_stream_ptr()),
              "pv_conv3d_pack_weights_multi_bf16")


def linear_wgrad_adam_bf16(x_bf16, dy, y_mask, param, exp_avg, exp_avg_sq, bf16_shadow, step: int, lr=5e-4,
                           betas=(0.9, 0.999), eps=1e-8):
    """fc1: gradient (dy ⊙ (y>0))^T x computed on the fly and applied by Adam in the same pass (no dw tensor)."""
    require_cuda(x_bf16, dy, y_mask, param, exp_avg, exp_avg_sq, bf16_shadow)
    m, k = x_bf16.shape
    n = param.shape[0]
    check(get_lib().pv_linear_wgrad_adam_bf16(ptr(x_bf16), ptr(dy), ptr(y_mask), ptr(param), ptr(exp_avg),
                                              ptr(exp_avg_sq), ptr(bf16_shadow), m, n, k, lr, betas[0], betas[1], eps,
                                              step, current_stream_ptr()), "pv_linear_wgrad_adam_bf16")


def linear_wgrad_adam_f32(x, dy, y_mask, param, exp_avg, exp_avg_sq, step: int, lr=5e-4, betas=(0.9, 0.999), eps=1e-8):
    """The f32 model's fc1: gradient (dy ⊙ (y>0))^T x from the f32 activations (exact products, f32 accumulation in batch order)
    applied by Adam in the same pass over p, m, v -- no gradient tensor (y_mask may be None: dy already gated)."""
    require_cuda(x, dy, y_mask, param, exp_avg, exp_avg_sq)
    if x.dtype != torch.float32 or not x.is_contiguous() or not dy.is_contiguous():
        raise TypeError("linear_wgrad_adam_f32: contiguous float32 x [M,K] and dy [M,N] expected")
    m, k = x.shape
    n = param.shape[0]
    check(get_lib().pv_linear_wgrad_adam_f32(ptr(x), ptr(dy), ptr(y_mask), ptr(param), ptr(exp_avg), ptr(exp_avg_sq), m, n, k, lr,
                                             betas[0], betas[1], eps, step, current_stream_ptr()), "pv_linear_wgrad_adam_f32")


def linear_wgrad_dx_adam_bf16(x_bf16, dy, y_mask, param, exp_avg, exp_avg_sq, bf16_shadow, step: int, lr=5e-4,
                              betas=(0.9, 0.999), eps=1e-8, need_dx=True, need_db=False, gate_dx_by_x=False,
                              moments_tiled=False):
    """fc1's whole backward in ONE pass over the matrix: weight gradient applied by Adam in place (as
    linear_wgrad_adam_bf16, bit-identical) AND dx = (dy ⊙ (y>0)) . W_old (bf16 [M, K]) from the weights it streams.
    gate_dx_by_x: dx is also multiplied by (x > 0), the ReLU derivative of the layer that produced x.
    moments_tiled: exp_avg / exp_avg_sq hold the [K/128][N][128] tile layout (moments_to_tiled)."""
    require_cuda(x_bf16, dy, y_mask, param, exp_avg, exp_avg_sq, bf16_shadow)
    m, k = x_bf16.shape
    n = param.shape[0]
    dx = torch.empty((m, k), dtype=torch.bfloat16, device=dy.device) if need_dx else None
    db = torch.empty(n, dtype=torch.float32, device=dy.device) if need_db else None
    check(get_lib().pv_linear_wgrad_dx_adam_bf16(ptr(x_bf16), ptr(dy), ptr(y_mask), ptr(param), ptr(exp_avg), ptr(exp_avg_sq),
                                                 ptr(bf16_shadow), ptr(dx), ptr(db), m, n, k, lr, betas[0], betas[1], eps,
                                                 step, int(bool(gate_dx_by_x)), int(bool(moments_tiled)),
                                                 current_stream_ptr()),
          "pv_linear_wgrad_dx_adam_bf16")
    return (dx, db) if need_db else dx


def linear_wgrad_dx_adam_dev_bf16(x_bf16, dy, y_mask, param, exp_avg, exp_avg_sq, bf16_shadow, scalars, need_db=False,
                                  gate_dx_by_x=False, moments_tiled=False):
    """linear_wgrad_dx_adam_bf16 with the step's Adam scalars in device memory (adam_scalars_advance)."""
    require_cuda(x_bf16, dy, y_mask, param, exp_avg, exp_avg_sq, bf16_shadow, scalars)
    m, k = x_bf16.shape
    n = param.shape[0]
    dx = torch.empty((m, k), dtype=torch.bfloat16, device=dy.device)
    db = torch.empty(n, dtype=torch.float32, device=dy.device) if need_db else None
    check(get_lib().pv_linear_wgrad_dx_adam_dev_bf16(ptr(x_bf16), ptr(dy), ptr(y_mask), ptr(param), ptr(exp_avg), ptr(exp_avg_sq),
                                                     ptr(bf16_shadow), ptr(dx), ptr(db), m, n, k, ptr(scalars),
                                                     int(bool(gate_dx_by_x)), int(bool(moments_tiled)), current_stream_ptr()),
          "pv_linear_wgrad_dx_adam_dev_bf16")
    return (dx, db) if need_db else dx


def linear_wgrad_dx_adam_tall_bf16(x_cols, g_all, param, exp_avg, exp_avg_sq, bf16_shadow, step: int, lr=5e-4, betas=(0.9, 0.999),
                                   eps=1e-8, grad_scale=1.0, need_dx=True, gate_dx_by_x=False, moments_tiled=False):
    """K-sharded fc1 (pv_linear_wgrad_dx_adam_tall_bf16): this rank's column shard updated by Adam from the gradient over ALL
    rows of the global batch (x_cols [M, K/W] bf16, g_all [M, N] f32, already gated), and dx_cols = g_all . W_old in the same pass."""
    require_cuda(x_cols, g_all, param, exp_avg, exp_avg_sq, bf16_shadow)
    m, k = x_cols.shape
    n = param.shape[0]
    dx = torch.empty((m, k), dtype=torch.bfloat16, device=g_all.device) if need_dx else None
    need = ctypes.c_size_t()
    check(get_lib().pv_linear_wgrad_dx_adam_tall_bf16_workspace_bytes(m, ctypes.byref(need)), "pv_linear_wgrad_dx_adam_tall_bf16_workspace_bytes")
    ws = torch.empty(need.value, dtype=torch.uint8, device=g_all.device)      # g_all as operand fragments (40 KB per 32 rows)
    check(get_lib().pv_linear_wgrad_dx_adam_tall_bf16(ptr(x_cols), ptr(g_all), ptr(param), ptr(exp_avg), ptr(exp_avg_sq),
                                                      ptr(bf16_shadow), ptr(dx), m, n, k, lr, betas[0], betas[1], eps, step,
                                                      float(grad_scale), int(bool(gate_dx_by_x)), int(bool(moments_tiled)), ptr(ws),
                                                      need.value, current_stream_ptr()),
          "pv_linear_wgrad_dx_adam_tall_bf16")
    return dx


def kshard_one_pass_supported(n: int, k: int) -> bool:
    return n <= 128 and n % 8 == 0 and k % 8 == 0


MOMENT_TILE = 128      # FD_KT of linear_bf16.hip: k-columns per workgroup of the one-pass fc1 backward


def moments_to_tiled(t: torch.Tensor) -> torch.Tensor:
    """Row-major [N, K] -> the tile layout [K/128][N][128] of pv_linear_wgrad_dx_adam_bf16(moments_tiled=1), as a tensor
    that keeps the shape [N, K] (only its bytes are permuted)."""
    n, k = t.shape
    return t.view(n, k // MOMENT_TILE, MOMENT_TILE).permute(1, 0, 2).contiguous().view(n, k)


def moments_to_rows(t: torch.Tensor) -> torch.Tensor:
    """Inverse of moments_to_tiled."""
    n, k = t.shape
    return t.view(k // MOMENT_TILE, n, MOMENT_TILE).permute(1, 0, 2).contiguous().view(n, k)


def fused_dx_update_supported(m: int, n: int, k: int, capturable: bool = False) -> bool:
    """m <= 32: pv_linear_wgrad_dx_adam_bf16 (or its device-scalar twin under a captured graph); more rows: the row-block form
    pv_linear_wgrad_dx_adam_tall_bf16 (host scalars only)."""
    return (m <= 32 or (m <= 4096 and not capturable)) and n <= 128 and n % 8 == 0 and k % 8 == 0


def linear_wgrad_bf16out(x_bf16, dy, y_mask, n: int) -> torch.Tensor:
    """fc1 weight gradient written directly as bf16 [N,K] (data-parallel wire format)."""
    require_cuda(x_bf16, dy, y_mask)
    m, k = x_bf16.shape
    dw = torch.empty((n, k), dtype=torch.bfloat16, device=dy.device)
    check(get_lib().pv_linear_wgrad_bf16out(ptr(x_bf16), ptr(dy), ptr(y_mask), ptr(dw), m, n, k, current_stream_ptr()),
          "pv_linear_wgrad_bf16out")
    return dw


def adam_step_bf16grad(param, grad_bf16, exp_avg, exp_avg_sq, step: int, lr=5e-4, betas=(0.9, 0.999), eps=1e-8,
                       bf16_shadow=None, grad_scale=1.0):
    require_cuda(param, grad_bf16, exp_avg, exp_avg_sq, bf16_shadow)
    check(get_lib().pv_adam_step_bf16grad(ptr(param), ptr(grad_bf16), ptr(exp_avg), ptr(exp_avg_sq), ptr(bf16_shadow),
                                          param.numel(), lr, betas[0], betas[1], eps, step, grad_scale,
                                          current_stream_ptr()), "pv_adam_step_bf16grad")


def scale_bias_relu_f32(x: torch.Tensor, bias: Optional[torch.Tensor] = None, alpha: float = 1.0, relu: bool = False) -> torch.Tensor:
    """act(alpha x + bias) over the rows of x [M, N] (pv_scale_bias_relu_f32)."""
    require_cuda(x, bias)
    x = x.contiguous()
    y = torch.empty_like(x)
    m = x.numel() // x.shape[-1]
    check(get_lib().pv_scale_bias_relu_f32(ptr(x), ptr(bias), ptr(y), m, x.shape[-1], float(alpha), int(bool(relu)),
                                           current_stream_ptr()), "pv_scale_bias_relu_f32")
    return y


def scale_f32(x: torch.Tensor, alpha: float) -> torch.Tensor:
    return scale_bias_relu_f32(x, None, alpha, False)


def clock_watch_launch(n_samples: int, sleep_units: int, stream) -> torch.Tensor:
    """Starts the one-wave clock watcher on `stream` (a torch.cuda.Stream other than the one the kernels of interest run on) and
    returns its sample buffer int64 [n_samples, 2] = (shader cycles, 100 MHz ticks); read it after stream.synchronize()."""
    buf = torch.zeros((n_samples, 2), dtype=torch.int64, device="cuda")
    check(get_lib().pv_clock_watch(ptr(buf), n_samples, sleep_units, ctypes.c_void_p(stream.cuda_stream)), "pv_clock_watch")
    return buf


def engine_clock_under(fn, seconds: float = 0.02) -> dict:
    """The engine clock (MHz) the device holds while `fn` (something that launches kernels on the current stream) loops for
    `seconds`: the one-wave watcher on a side stream, samples taken well inside the loop.  sysfs reads a ~10 ms average and cannot
    see a 70 us kernel; the conv kernels run at ~1.7-1.8 GHz where the idle device and a plain copy read 2.4."""
    import time
    side = torch.cuda.Stream()
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    n = int((seconds + 0.012) * 1e6 / 1.1) + 1000
    buf = clock_watch_launch(n, 40, side)
    time.sleep(0.002)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        fn()
    torch.cuda.synchronize()
    s = buf.cpu().numpy().astype(np.float64)
    s = s[s[:, 1] > 0]
    t_us = (s[:, 1] - s[0, 1]) / 100.0
    dt, dr = np.diff(s[:, 0]), np.diff(s[:, 1])
    ok = (dr > 0) & (t_us[1:] > 6000) & (t_us[1:] < 2000 + seconds * 1e6 - 3000)
    mhz = dt[ok] / dr[ok] * 100.0
    if len(mhz) < 50:
        return {"samples": int(len(mhz))}
    return {"median_MHz": round(float(np.median(mhz))), "p10_MHz": round(float(np.percentile(mhz, 10))),
            "p90_MHz": round(float(np.percentile(mhz, 90))), "samples": int(len(mhz))}


def swap01_segments(x: torch.Tensor) -> torch.Tensor:
    """x [n0, n1, seg] contiguous -> [n1, n0, seg] contiguous (pv_swap01_segments; segments of a multiple of 16 bytes): the
    staging copy of an all-to-all whose chunks are column slices."""
    require_cuda(x)
    if x.dim() != 3 or not x.is_contiguous() or (x.shape[2] * x.element_size()) % 16:
        raise TypeError("swap01_segments: a contiguous [n0, n1, seg] tensor with segments of a multiple of 16 bytes")
    out = torch.empty((x.shape[1], x.shape[0], x.shape[2]), dtype=x.dtype, device=x.device)
    check(get_lib().pv_swap01_segments(ptr(x), ptr(out), x.shape[0], x.shape[1], x.shape[2] * x.element_size(), current_stream_ptr()),
          "pv_swap01_segments")
    return out


def cast_f32_to_bf16(x: torch.Tensor) -> torch.Tensor:
    """bf16 (round to nearest even) copy of a contiguous f32 tensor (pv_cast_f32_to_bf16)."""
    require_cuda(x)
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    check(get_lib().pv_cast_f32_to_bf16(ptr(x), ptr(out), x.numel(), current_stream_ptr()), "pv_cast_f32_to_bf16")
    return out


def embedding_fwd(table: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    require_cuda(table, ids)
    ids = ids.to(torch.int64).contiguous()
    out = torch.empty((ids.numel(), table.shape[1]), dtype=torch.float32, device=table.device)
    check(get_lib().pv_embedding_fwd_f32(ptr(table), ptr(ids), ptr(out), ids.numel(), table.shape[1], table.shape[0],
                                         current_stream_ptr()), "pv_embedding_fwd_f32")
    return out


def embedding_bwd(dout: torch.Tensor, ids: torch.Tensor, n_rows: int) -> torch.Tensor:
    require_cuda(dout, ids)
    ids = ids.to(torch.int64).contiguous()
    dtable = torch.empty((n_rows, dout.shape[1]), dtype=torch.float32, device=dout.device)
    check(get_lib().pv_embedding_bwd_f32(ptr(dout), ptr(ids), ptr(dtable), ids.numel(), dout.shape[1], n_rows,
                                         current_stream_ptr()), "pv_embedding_bwd_f32")
    return dtable


# ---- general Conv3D / MaxPool3d / MSE (optical-flow notebook model, Conv3dMaxPool) -----------------------------------
def _triple(v):
    return (v, v, v) if isinstance(v, int) else tuple(int(a) for a in v)


def conv_geom(batch, c_in, c_out, t, h, w, kernel, stride=1, padding=0) -> Conv3dGeom:
    return Conv3dGeom(batch, c_in, c_out, t, h, w, *_triple(kernel), *_triple(stride), *_triple(padding))


def relu_gate_f32(dy: torch.Tensor, y: torch.Tensor, want_max: bool = False) -> torch.Tensor:
    """dy where y > 0, else 0 (the backward of F.relu, model.py:117-120), f32.  want_max: -> (out, state): the pass also
    leaves the bits of the largest |out| in state[0] -- the scale pack_split2_ncdhw_f32_to_ndhwc_f16 needs, found without a pass
    of its own (hand it over as maxabs_state)."""
    require_cuda(dy, y)
    if dy.dtype != torch.float32 or y.dtype != torch.float32 or dy.numel() != y.numel() or dy.numel() % 4:
        raise TypeError("relu_gate_f32: two float32 tensors of equal size (a multiple of 4 elements)")
    dy, y = dy.contiguous(), y.contiguous()
    out = torch.empty_like(dy)
    if want_max:
        state = torch.empty(3, dtype=torch.float32, device=dy.device)
        check(get_lib().pv_relu_gate_max_f32(ptr(dy), ptr(y), ptr(out), dy.numel(), ptr(state), current_stream_ptr()),
              "pv_relu_gate_max_f32")
        return out, state
    check(get_lib().pv_relu_gate_f32(ptr(dy), ptr(y), ptr(out), dy.numel(), current_stream_ptr()), "pv_relu_gate_f32")
    return out


def conv3d_general_fwd_f32(x, weight, bias, stride=1, padding=0, relu=False):
    require_cuda(x, weight, bias)
    b, ci, t, h, w = x.shape
    co = weight.shape[0]
    g = conv_geom(b, ci, co, t, h, w, tuple(weight.shape[2:]), stride, padding)
    y = torch.empty((b, co) + g.out_shape(), dtype=torch.float32, device=x.device)
    check(get_lib().pv_conv3d_general_fwd_f32(ptr(x), ptr(weight), ptr(bias), ptr(y), ctypes.byref(g), int(relu),
                                              current_stream_ptr()), "pv_conv3d_general_fwd_f32")
    return y


def conv3d_general_bwd_data_f32(dy, y_mask, weight, x_shape, stride=1, padding=0, x_mask=None):
    require_cuda(dy, y_mask, weight, x_mask)
    b, ci, t, h, w = x_shape
    g = conv_geom(b, ci, weight.shape[0], t, h, w, tuple(weight.shape[2:]), stride, padding)
    dx = torch.empty(x_shape, dtype=torch.float32, device=dy.device)
    check(get_lib().pv_conv3d_general_bwd_data_f32(ptr(dy), ptr(y_mask), ptr(weight), ptr(dx), ptr(x_mask), ctypes.byref(g),
                                                   current_stream_ptr()), "pv_conv3d_general_bwd_data_f32")
    return dx


def conv3d_general_bwd_weight_f32(x, dy, y_mask, weight_shape, stride=1, padding=0, need_bias=True):
    require_cuda(x, dy, y_mask)
    b, ci, t, h, w = x.shape
    g = conv_geom(b, ci, weight_shape[0], t, h, w, tuple(weight_shape[2:]), stride, padding)
    nbytes = ctypes.c_size_t(0)
    check(get_lib().pv_conv3d_general_bwd_weight_workspace_bytes(ctypes.byref(g), ctypes.byref(nbytes)),
          "pv_conv3d_general_bwd_weight_workspace_bytes")
    ws = _workspace("conv3d_general_wgrad", nbytes.value, x.device)
    dw = torch.empty(weight_shape, dtype=torch.float32, device=x.device)
    db = torch.empty((weight_shape[0],), dtype=torch.float32, device=x.device) if need_bias else None
    check(get_lib().pv_conv3d_general_bwd_weight_f32(ptr(x), ptr(dy), ptr(y_mask), ptr(dw), ptr(db), ctypes.byref(g),
                                                     ptr(ws), nbytes.value, current_stream_ptr()),
          "pv_conv3d_general_bwd_weight_f32")
    return dw, db


# ------------------------------------------------------------------------------------------------
# Conv2d / ConvTranspose2d 3x3, exact f32, for six models: experiments/002 (conv2d_*, 17 / 32 -> 32 / 4 channels),
# experiments/001 (conv2d144_*, 144 -> 144, + MaxPool2d(3)), notebooks/16_maxpool.ipynb (conv2d_ae_* / convt2d_ae_*, + pool,
# cropped normalised MSE), notebooks/14, 15 (conv2d_s2_* / convt2d_s2_*, stride 2, windowed normalised MSE), notebooks/10
# (conv2d_wide_*, conv2d_head_s2_*: padded 64 / 128 channels, stripe first layer) and notebooks/09 (conv2d_wide_s2_*,
# convt2d_wide_s2_*, convt2d_head_*: the same widths at stride 2, MSE over a window of the prediction); further down,
# notebooks/07 (conv2d_s2_frame_horizon_*, convt2d_s2_frames_*: the per-frame first layer and ConvTranspose2d 128 -> 32).
#
# A family of entry points is described once, by a _ConvFamily record (its plain forward / data gradient / weight gradient)
# and, where it has them, a _PoolFamily record (the same three passes with MaxPool2d(3) fused).  _conv_fwd, _conv_bwd_data,
# _conv_bwd_weight, _pool_*, _counts_* and _mse_norm are the only implementations; the public functions below them are
# one-line calls, for the Conv3d families of notebooks 12 and 08 further down as well.  A new family is a new record (its
# shape rule) plus its one-line functions, and its argtypes from the shared lists of _lib.py; a new pass is written once here.
# tests/test_conv2d_glue_cpu.py pins what each wrapper hands to the C ABI.
# ------------------------------------------------------------------------------------------------
C144 = 144


def _f32_contig(*ts):
    for t in ts:
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise TypeError("conv2d kernels take contiguous float32 tensors")


def _u8_contig(who, codes):
    if codes.dtype != torch.uint8 or not codes.is_contiguous():
        raise TypeError(f"{who}: codes must be a contiguous uint8 tensor")


def _counts_contig(who, *ts):
    for t in ts:
        if t.dtype not in (torch.int16, torch.float32) or not t.is_contiguous():
            raise TypeError(f"{who}: counts must be contiguous int16 or float32 tensors, got {t.dtype}")


def _check_bias(who, bias, c_out):
    if bias is not None and tuple(bias.shape) != (c_out,):
        raise ValueError(f"{who}: bias [{c_out}] expected, got {tuple(bias.shape)}")


def _check_xy_coords(who, x_coords, y_coords, b, h, w):
    if tuple(x_coords.shape) != (b, w) or tuple(y_coords.shape) != (b, h):
        raise ValueError(f"{who}: x_coords [{b}, {w}] and y_coords [{b}, {h}] expected, got {tuple(x_coords.shape)} / "
                         f"{tuple(y_coords.shape)}")


def _check_coords(who, sat, x_coords, y_coords, t_per_example):
    n, h, w, c = sat.shape
    if not (c == 12 and t_per_example > 0 and n % t_per_example == 0):
        raise ValueError(f"{who}: sat [N, H, W, 12] with N a multiple of t_per_example={t_per_example}, got "
                         f"{tuple(sat.shape)}")
    _check_xy_coords(who, x_coords, y_coords, n // t_per_example, h, w)


def _check_sat001(who, sat, x_coords, y_coords, n_frames):
    if not (sat.dim() == 5 and sat.shape[4] == 1):
        raise ValueError(f"{who}: sat_data [B, T, H, W, 1] expected, got {tuple(sat.shape)}")
    b, t, h, w, _ = sat.shape
    if not 0 < n_frames <= t:
        raise ValueError(f"{who}: n_frames={n_frames} must lie in 1..T={t}")
    if h < 5 or w < 5:
        raise ValueError(f"{who}: images of at least 5 x 5 expected, got {h} x {w}")
    _check_xy_coords(who, x_coords, y_coords, b, h, w)
    return b, t, h, w


def _check_counts(who, history, flow_pred, horizon):
    if not (history.dim() == 4 and history.shape[1] == 4):
        raise ValueError(f"{who}: history [N, 4, H, W] expected, got {tuple(history.shape)}")
    n, _, h, w = history.shape
    if tuple(flow_pred.shape) != (n, h, w) or tuple(horizon.shape) != (n,):
        raise ValueError(f"{who}: flow prediction [{n}, {h}, {w}] and horizon [{n}] expected, got "
                         f"{tuple(flow_pred.shape)} / {tuple(horizon.shape)}")
    require_cuda(history, flow_pred, horizon)
    _counts_contig(who, history, flow_pred)
    _f32_contig(horizon)
    return n, h, w


def _check_c32(who, x_shape, weight_shape):
    n, ci, h, w = x_shape
    if not (len(weight_shape) == 4 and tuple(weight_shape[1:]) == (ci, 3, 3)):
        raise ValueError(f"{who}: weight [C_out, {ci}, 3, 3] expected for x {tuple(x_shape)}, got {tuple(weight_shape)}")


def _check_c144(who, x_shape, weight_shape, pooled=False):
    if not (len(x_shape) == 4 and x_shape[1] == C144):
        raise ValueError(f"{who}: x [N, 144, H, W] expected, got {tuple(x_shape)}")
    if tuple(weight_shape) != (C144, C144, 3, 3):
        raise ValueError(f"{who}: weight [144, 144, 3, 3] expected, got {tuple(weight_shape)}")
    lo = 5 if pooled else 3
    if x_shape[2] < lo or x_shape[3] < lo:
        raise ValueError(f"{who}: images of at least {lo} x {lo} expected, got {tuple(x_shape)}")


def _check_c144_pooled(who, x_shape, weight_shape):
    _check_c144(who, x_shape, weight_shape, True)


def _check_ae(who, x_shape, weight_shape):
    if not (len(x_shape) == 4 and len(weight_shape) == 4 and tuple(weight_shape[1:]) == (x_shape[1], 3, 3)):
        raise ValueError(f"{who}: x [N, C_in, H, W] and weight [C_out, C_in, 3, 3] expected, got {tuple(x_shape)} / "
                         f"{tuple(weight_shape)}")


def _check_aet(who, x_shape, weight_shape):
    if not (len(x_shape) == 4 and len(weight_shape) == 4 and weight_shape[0] == x_shape[1]
            and tuple(weight_shape[2:]) == (3, 3)):
        raise ValueError(f"{who}: x [N, C_in, H, W] and weight [C_in, C_out, 3, 3] expected, got {tuple(x_shape)} / "
                         f"{tuple(weight_shape)}")


AE_P2_PAIR = (32, 32)                     # (c_in, c_out) of pv_conv2d_ae_p2_*


def _check_ae_p2(who, x_shape, weight_shape):
    _check_ae(who, x_shape, weight_shape)
    if (x_shape[1], weight_shape[0]) != AE_P2_PAIR:
        raise ValueError(f"{who}: (C_in, C_out) = (32, 32) expected with padding 2, got ({x_shape[1]}, {weight_shape[0]})")
    if min(x_shape[2:]) < 1 or x_shape[3] + 2 > WIDE_MAX_W:
        raise ValueError(f"{who}: a non-empty plane whose output is at most {WIDE_MAX_W} columns wide expected, got "
                         f"{x_shape[2]} x {x_shape[3]}")


def _pooled_shape(n, c, h, w):
    return (n, c, (h - 2) // 3, (w - 2) // 3)


def _pooled_shape_c(n, c, h, w):
    if h < 5 or w < 5:
        raise ValueError(f"images of at least 5 x 5 expected (one whole 3x3 pool window after the 3x3 conv), got {h} x {w}")
    return _pooled_shape(n, c, h, w)


WIDE_PAIRS = ((64, 128), (128, 128))      # (c_in, c_out) of pv_conv2d_wide_*
WIDE_MAX_W = 128
STRIPE_C_OUT = 64
STRIPE_MAX_HIST = 7


def _check_wide(who, x_shape, weight_shape, pad):
    _check_ae(who, x_shape, weight_shape)
    n, ci, h, w = x_shape
    if (ci, weight_shape[0]) not in WIDE_PAIRS:
        raise ValueError(f"{who}: (C_in, C_out) = (64, 128) or (128, 128) expected, got ({ci}, {weight_shape[0]})")
    if min(h, w) + 2 * pad < 3 or w > WIDE_MAX_W:
        raise ValueError(f"{who}: planes of at least {max(3 - 2 * pad, 1)} rows / columns and at most {WIDE_MAX_W} columns "
                         f"expected, got {h} x {w}")


def _check_head(who, x_shape, weight_shape):
    _check_ae(who, x_shape, weight_shape)
    if weight_shape[0] != 1 or x_shape[2] < 1 or x_shape[3] < 1:
        raise ValueError(f"{who}: weight [1, C_in, 3, 3] and a non-empty plane expected, got {tuple(weight_shape)} / "
                         f"{tuple(x_shape)}")


def _check_wide_s2(who, x_shape, weight_shape):
    _check_ae(who, x_shape, weight_shape)
    n, ci, h, w = x_shape
    if (ci, weight_shape[0]) not in WIDE_PAIRS:
        raise ValueError(f"{who}: (C_in, C_out) = (64, 128) or (128, 128) expected, got ({ci}, {weight_shape[0]})")
    if min(h, w) < 3 or w > WIDE_MAX_W:
        raise ValueError(f"{who}: planes of at least 3 x 3 and at most {WIDE_MAX_W} columns expected, got {h} x {w}")


def _check_widet_s2(who, x_shape, weight_shape):
    _check_aet(who, x_shape, weight_shape)
    n, ci, h, w = x_shape
    if (ci, weight_shape[1]) != (128, 128):
        raise ValueError(f"{who}: (C_in, C_out) = (128, 128) expected, got ({ci}, {weight_shape[1]})")
    if min(h, w) < 1 or 2 * w + 1 > WIDE_MAX_W:
        raise ValueError(f"{who}: a non-empty plane whose output is at most {WIDE_MAX_W} columns wide expected, got {h} x {w}")


def _check_headt(who, x_shape, weight_shape):
    _check_aet(who, x_shape, weight_shape)
    if weight_shape[1] != 1 or x_shape[2] < 1 or x_shape[3] < 1 or x_shape[3] > WIDE_MAX_W:
        raise ValueError(f"{who}: weight [C_in, 1, 3, 3] and a non-empty plane of at most {WIDE_MAX_W} columns expected, got "
                         f"{tuple(weight_shape)} / {tuple(x_shape)}")


def head_s2_out(side):
    """Side of a 3x3 stride-2 padding-2 Conv2d's output."""
    return (side + 1) // 2 + 1


def s2_out(side):
    """Side of a 3x3 stride-2 Conv2d's output."""
    return (side - 3) // 2 + 1


class _ConvFamily(NamedTuple):
    """One family of plain entry points, 2-D or 3-D: pv_{stem}_{fwd,bwd_data,bwd_weight}_f32 and
    pv_{stem}_bwd_weight_workspace_bytes."""
    stem: str                       # also names the weight gradient's workspace, "{stem}_wgrad" (a captured graph pins by key)
    shape: Callable                 # (who, x_shape, weight_shape) -> (every pass's integers (n, c_in, c_out, sides.., padding..),
    #                                 the output's shape); raises ValueError
    ws_args: tuple = ()             # the workspace query's arguments after those integers: the "pooled" flag, 0 here
    out_hw: Callable = None         # 2-D: (h, w) of the input -> (h, w) of the output, for the synthesised first layers
    pad_args: tuple = ()            # 2-D: the padding of a padded family, which follows (n, c_in, c_out, h, w)


def _conv2d_family(stem, check_channels, out_hw, c_out_axis=0, ws_args=(), pad_args=()):
    """A 2-D family from its channel rule (who, x_shape, weight_shape), which raises ValueError, and its output rule;
    c_out_axis of the weight: 0 in Conv2d's [C_out, C_in, 3, 3], 1 in ConvTranspose2d's [C_in, C_out, 3, 3]."""
    def shape(who, x_shape, weight_shape):
        check_channels(who, x_shape, weight_shape)
        n, ci, h, w = x_shape
        co = weight_shape[c_out_axis]
        return (n, ci, co, h, w, *pad_args), (n, co, *out_hw(h, w))
    return _ConvFamily(stem, shape, ws_args, out_hw, pad_args)


class _PoolFamily(NamedTuple):
    """The conv + MaxPool2d(3) passes of a family, pv_{stem}_pool_{fwd,bwd_data,bwd_weight}_f32; the weight gradient takes
    the plain family's workspace, queried with the "pooled" flag 1."""
    stem: str
    check_channels: Callable        # (who, x_shape, weight_shape): raises ValueError; the pooled passes need a bias
    pooled_shape: Callable          # (n, c_out, h, w) -> shape of the pooled output
    fwd_workspace: bool             # the forward has pv_{stem}_pool_fwd_workspace_bytes and takes (workspace, bytes)


def _valid_hw(h, w):
    return h - 2, w - 2         # not clamped: a plane under 3 rows fails in torch.empty


def _s2_hw(h, w):
    return max(s2_out(h), 0), max(s2_out(w), 0)


_CONV2D = _conv2d_family("conv2d", _check_c32, _valid_hw)
_CONV2D144 = _conv2d_family("conv2d144", _check_c144, _valid_hw, ws_args=(0,))
_CONV2D_AE = _conv2d_family("conv2d_ae", _check_ae, _valid_hw, ws_args=(0,))
# notebook 11: the padded 32 -> 32 layer, a record of its own (its stem names its entry points and its workspace)
_CONV2D_AE_P2 = _conv2d_family("conv2d_ae_p2", _check_ae_p2, lambda h, w: (h + 2, w + 2))
_CONVT2D_AE = _conv2d_family("convt2d_ae", _check_aet, lambda h, w: (h + 2, w + 2), c_out_axis=1)
_CONV2D_S2 = _conv2d_family("conv2d_s2", _check_ae, _s2_hw)
_CONVT2D_S2 = _conv2d_family("convt2d_s2", _check_aet, lambda h, w: (2 * h + 1, 2 * w + 1), c_out_axis=1)
# notebook 10: the padded wide family is one stem with a record per padding (the padding goes to every pass and to the
# workspace query); the stride-2 head maps a side s to (s + 1) // 2 + 1
_CONV2D_WIDE_P0 = _conv2d_family("conv2d_wide", lambda *a: _check_wide(*a, pad=0), _valid_hw, pad_args=(0,))
_CONV2D_WIDE_P2 = _conv2d_family("conv2d_wide", lambda *a: _check_wide(*a, pad=2), lambda h, w: (h + 2, w + 2), pad_args=(2,))
_CONV2D_HEAD_S2 = _conv2d_family("conv2d_head_s2", lambda *a: _check_head(*a), lambda h, w: (head_s2_out(h), head_s2_out(w)))
# notebook 09: the stride-2 64 / 128-channel layers and the one-output-channel ConvTranspose2d head (stride 1)
_CONV2D_WIDE_S2 = _conv2d_family("conv2d_wide_s2", _check_wide_s2, _s2_hw)
_CONVT2D_WIDE_S2 = _conv2d_family("convt2d_wide_s2", _check_widet_s2, lambda h, w: (2 * h + 1, 2 * w + 1), c_out_axis=1)
_CONVT2D_HEAD = _conv2d_family("convt2d_head", _check_headt, lambda h, w: (h + 2, w + 2), c_out_axis=1)
_CONV2D144_POOL = _PoolFamily("conv2d144", _check_c144_pooled, _pooled_shape, False)
_CONV2D_AE_POOL = _PoolFamily("conv2d_ae", _check_ae, _pooled_shape_c, True)


def _wgrad_ws(family, device, *dims):
    """(buffer, bytes) for pv_{family}_bwd_weight_*.  Each family keeps its own workspace key: a captured graph pins
    workspaces by key."""
    query = f"pv_{family}_bwd_weight_workspace_bytes"
    nbytes = ctypes.c_size_t(0)
    check(getattr(get_lib(), query)(*dims, ctypes.byref(nbytes)), query)
    return _workspace(f"{family}_wgrad", nbytes.value, device), nbytes.value


def _grads_out(weight_shape, c_out, device):
    return (torch.empty(tuple(weight_shape), dtype=torch.float32, device=device),
            torch.empty((c_out,), dtype=torch.float32, device=device))


def _check_dy(who, dy, dy_gate, y_shape):
    if tuple(dy.shape) != y_shape or (dy_gate is not None and tuple(dy_gate.shape) != y_shape):
        raise ValueError(f"{who}: dy / dy_gate {y_shape} expected, got {tuple(dy.shape)}")


# ---- the plain passes ----
def _conv_fwd(fam, x, weight, bias, relu):
    who = f"{fam.stem}_fwd_f32"
    dims, y_shape = fam.shape(who, x.shape, weight.shape)
    _check_bias(who, bias, dims[2])
    require_cuda(x, weight, bias)
    _f32_contig(x, weight, bias)
    y = torch.empty(y_shape, dtype=torch.float32, device=x.device)
    check(getattr(get_lib(), "pv_" + who)(ptr(x), ptr(weight), ptr(bias), ptr(y), *dims, int(relu), current_stream_ptr()),
          "pv_" + who)
    return y


def _conv_bwd_data(fam, dy, dy_gate, weight, x_gate, x_shape):
    who = f"{fam.stem}_bwd_data_f32"
    dims, y_shape = fam.shape(who, x_shape, weight.shape)
    _check_dy(who, dy, dy_gate, y_shape)
    if x_gate is not None and tuple(x_gate.shape) != tuple(x_shape):
        raise ValueError(f"{who}: x_gate {tuple(x_shape)} expected")
    require_cuda(dy, dy_gate, weight, x_gate)
    _f32_contig(dy, dy_gate, weight, x_gate)
    dx = torch.empty(tuple(x_shape), dtype=torch.float32, device=dy.device)
    check(getattr(get_lib(), "pv_" + who)(ptr(dy), ptr(dy_gate), ptr(weight), ptr(dx), ptr(x_gate), *dims,
                                          current_stream_ptr()), "pv_" + who)
    return dx


def _conv_bwd_weight(fam, x, dy, dy_gate, weight_shape):
    who = f"{fam.stem}_bwd_weight_f32"
    dims, y_shape = fam.shape(who, x.shape, weight_shape)
    _check_dy(who, dy, dy_gate, y_shape)
    require_cuda(x, dy, dy_gate)
    _f32_contig(x, dy, dy_gate)
    ws, nbytes = _wgrad_ws(fam.stem, x.device, *dims, *fam.ws_args)
    dw, db = _grads_out(weight_shape, dims[2], x.device)
    check(getattr(get_lib(), "pv_" + who)(ptr(x), ptr(dy), ptr(dy_gate), ptr(dw), ptr(db), *dims, ptr(ws), nbytes,
                                          current_stream_ptr()), "pv_" + who)
    return dw, db


# ---- conv + MaxPool2d(3): the forward also returns one uint8 code per pooled output, which the gradients take ----
def _check_pooled(who, pool, dy_pooled, codes, n, co, h, w):
    p_shape = pool.pooled_shape(n, co, h, w)
    if tuple(dy_pooled.shape) != p_shape or tuple(codes.shape) != p_shape:
        raise ValueError(f"{who}: dy_pooled / codes {p_shape} expected, got {tuple(dy_pooled.shape)} / "
                         f"{tuple(codes.shape)}")


def _pool_fwd(pool, x, weight, bias):
    who = f"{pool.stem}_pool_fwd_f32"
    pool.check_channels(who, x.shape, weight.shape)
    n, c, h, w = x.shape
    co = weight.shape[0]
    if bias is None or tuple(bias.shape) != (co,):
        raise ValueError(f"{who}: bias [{co}] expected")
    require_cuda(x, weight, bias)
    _f32_contig(x, weight, bias)
    y = torch.empty(pool.pooled_shape(n, co, h, w), dtype=torch.float32, device=x.device)
    codes = torch.empty(y.shape, dtype=torch.uint8, device=x.device)
    ws_args = ()
    if pool.fwd_workspace:
        query = f"pv_{pool.stem}_pool_fwd_workspace_bytes"
        nbytes = ctypes.c_size_t(0)
        check(getattr(get_lib(), query)(n, c, co, h, w, ctypes.byref(nbytes)), query)
        ws = _workspace(f"{pool.stem}_pool_fwd", nbytes.value, x.device) if nbytes.value else None
        ws_args = (ptr(ws), nbytes.value)
    check(getattr(get_lib(), "pv_" + who)(ptr(x), ptr(weight), ptr(bias), ptr(y), ptr(codes), n, c, co, h, w, *ws_args,
                                          current_stream_ptr()), "pv_" + who)
    return y, codes


def _pool_bwd_data(pool, dy_pooled, codes, weight, x_gate, x_shape):
    who = f"{pool.stem}_pool_bwd_data_f32"
    pool.check_channels(who, x_shape, weight.shape)
    n, c, h, w = x_shape
    co = weight.shape[0]
    _check_pooled(who, pool, dy_pooled, codes, n, co, h, w)
    if x_gate is not None and tuple(x_gate.shape) != tuple(x_shape):
        raise ValueError(f"{who}: x_gate {tuple(x_shape)} expected")
    require_cuda(dy_pooled, codes, weight, x_gate)
    _f32_contig(dy_pooled, weight, x_gate)
    _u8_contig(who, codes)
    dx = torch.empty(tuple(x_shape), dtype=torch.float32, device=dy_pooled.device)
    check(getattr(get_lib(), "pv_" + who)(ptr(dy_pooled), ptr(codes), ptr(weight), ptr(dx), ptr(x_gate), n, c, co, h, w,
                                          current_stream_ptr()), "pv_" + who)
    return dx


def _pool_bwd_weight(pool, x, dy_pooled, codes, weight_shape):
    who = f"{pool.stem}_pool_bwd_weight_f32"
    pool.check_channels(who, x.shape, weight_shape)
    n, c, h, w = x.shape
    co = weight_shape[0]
    _check_pooled(who, pool, dy_pooled, codes, n, co, h, w)
    require_cuda(x, dy_pooled, codes)
    _f32_contig(x, dy_pooled)
    _u8_contig(who, codes)
    ws, nbytes = _wgrad_ws(pool.stem, x.device, n, c, co, h, w, 1)
    dw, db = _grads_out(weight_shape, co, x.device)
    check(getattr(get_lib(), "pv_" + who)(ptr(x), ptr(dy_pooled), ptr(codes), ptr(dw), ptr(db), n, c, co, h, w, ptr(ws),
                                          nbytes, current_stream_ptr()), "pv_" + who)
    return dw, db


# ---- the raw-counts first layer of notebooks 14-16, on its plain family's output rule and weight-gradient workspace ----
def _counts_fwd(fam, history, flow_pred, horizon, weight, bias):
    who = f"{fam.stem}_counts_fwd_f32"
    n, h, w = _check_counts(who, history, flow_pred, horizon)
    co = weight.shape[0]
    if tuple(weight.shape) != (co, 6, 3, 3):
        raise ValueError(f"{who}: weight [C_out, 6, 3, 3] expected, got {tuple(weight.shape)}")
    if bias is None or tuple(bias.shape) != (co,):
        raise ValueError(f"{who}: bias [{co}] expected")
    require_cuda(weight, bias)
    _f32_contig(weight, bias)
    # clamped, unlike the plain forward: an undersized plane reaches the entry point, which names the smallest it takes
    oh, ow = fam.out_hw(h, w)
    y = torch.empty((n, co, max(oh, 0), max(ow, 0)), dtype=torch.float32, device=history.device)
    check(getattr(get_lib(), "pv_" + who)(ptr(history), int(history.dtype == torch.int16), ptr(flow_pred),
                                          int(flow_pred.dtype == torch.int16), ptr(horizon), ptr(weight), ptr(bias), ptr(y),
                                          n, h, w, co, current_stream_ptr()), "pv_" + who)
    return y


def _counts_bwd_weight(fam, history, flow_pred, horizon, dy, weight_shape):
    who = f"{fam.stem}_counts_bwd_weight_f32"
    n, h, w = _check_counts(who, history, flow_pred, horizon)
    co = weight_shape[0]
    y_shape = (n, co, *fam.out_hw(h, w))
    if tuple(weight_shape) != (co, 6, 3, 3) or tuple(dy.shape) != y_shape:
        raise ValueError(f"{who}: weight {(co, 6, 3, 3)} and dy {y_shape} expected, got {tuple(weight_shape)} / "
                         f"{tuple(dy.shape)}")
    require_cuda(dy)
    _f32_contig(dy)
    ws, nbytes = _wgrad_ws(fam.stem, history.device, n, 6, co, h, w, *fam.pad_args, *fam.ws_args)
    dw, db = _grads_out(weight_shape, co, history.device)
    check(getattr(get_lib(), "pv_" + who)(ptr(history), int(history.dtype == torch.int16), ptr(flow_pred),
                                          int(flow_pred.dtype == torch.int16), ptr(horizon), ptr(dy), ptr(dw), ptr(db), n, h,
                                          w, co, ptr(ws), nbytes, current_stream_ptr()), "pv_" + who)
    return dw, db


def _mse_norm(name, y_hat, target, window, need_grad):
    """pv_{name}_f32 and the workspace "{name}": window = () for the crop form, whose entry point matches the sides itself,
    (row0, col0) for the window form."""
    who = name + "_f32"
    if not (y_hat.dim() == 3 and target.dim() == 3 and target.shape[0] == y_hat.shape[0]):
        raise ValueError(f"{who}: y_hat [N, P, Q] and target [N, T, U] expected, got {tuple(y_hat.shape)} / "
                         f"{tuple(target.shape)}")
    require_cuda(y_hat, target)
    _f32_contig(y_hat)
    _counts_contig(who, target)
    n, oh, ow = y_hat.shape
    loss = torch.empty((1,), dtype=torch.float32, device=y_hat.device)
    grad = torch.empty_like(y_hat) if need_grad else None
    ws = _workspace(name, 4 * n, y_hat.device)
    check(getattr(get_lib(), "pv_" + who)(ptr(y_hat), ptr(target), int(target.dtype == torch.int16), n, oh, ow,
                                          target.shape[1], target.shape[2], *map(int, window), ptr(loss), ptr(grad), ptr(ws),
                                          4 * n, current_stream_ptr()), "pv_" + who)
    return loss, grad


# ---- experiments/002_cnn_processes_single_sat_image_then_rnn.py (csrc/conv2d_f32.hip) ----
def conv2d_coords_fwd_f32(sat, x_coords, y_coords, weight, bias, t_per_example):
    """relu(conv2d(cat(sat.permute(0, 3, 1, 2), 5 synthesised channels), weight) + bias) with sat [N, H, W, 12],
    x_coords [N / t, W], y_coords [N / t, H]: the 17-channel input is built inside the kernel.  Returns [N, C_out, H-2, W-2]."""
    who = "conv2d_coords_fwd_f32"
    _check_coords(who, sat, x_coords, y_coords, t_per_example)
    n, h, w, c = sat.shape
    if not (weight.dim() == 4 and tuple(weight.shape[1:]) == (17, 3, 3)):
        raise ValueError(f"{who}: weight [C_out, 17, 3, 3] expected, got {tuple(weight.shape)}")
    co = weight.shape[0]
    _check_bias(who, bias, co)
    require_cuda(sat, x_coords, y_coords, weight, bias)
    _f32_contig(sat, x_coords, y_coords, weight, bias)
    y = torch.empty((n, co, h - 2, w - 2), dtype=torch.float32, device=sat.device)
    check(getattr(get_lib(), "pv_" + who)(ptr(sat), ptr(x_coords), ptr(y_coords), ptr(weight), ptr(bias), ptr(y), n,
                                          t_per_example, h, w, co, current_stream_ptr()), "pv_" + who)
    return y


def conv2d_coords_bwd_weight_f32(sat, x_coords, y_coords, dy, t_per_example, weight_shape):
    """(dw, dbias) of conv2d_coords_fwd_f32's conv from its pre-activation gradient dy, re-synthesising the input."""
    who = "conv2d_coords_bwd_weight_f32"
    _check_coords(who, sat, x_coords, y_coords, t_per_example)
    n, h, w, _ = sat.shape
    co = weight_shape[0]
    if tuple(weight_shape) != (co, 17, 3, 3) or tuple(dy.shape) != (n, co, h - 2, w - 2):
        raise ValueError(f"{who}: weight {(co, 17, 3, 3)} and dy {(n, co, h - 2, w - 2)} expected, got "
                         f"{tuple(weight_shape)} / {tuple(dy.shape)}")
    require_cuda(sat, x_coords, y_coords, dy)
    _f32_contig(sat, x_coords, y_coords, dy)
    ws, nbytes = _wgrad_ws("conv2d", sat.device, n, 17, co, h, w)
    dw, db = _grads_out(weight_shape, co, sat.device)
    check(getattr(get_lib(), "pv_" + who)(ptr(sat), ptr(x_coords), ptr(y_coords), ptr(dy), ptr(dw), ptr(db), n,
                                          t_per_example, h, w, co, ptr(ws), nbytes, current_stream_ptr()), "pv_" + who)
    return dw, db


def conv2d_fwd_f32(x, weight, bias, relu=True):
    """conv2d(x, weight) + bias (+ ReLU) for x [N, 32, H, W] -> [N, C_out, H-2, W-2], C_out = 32 or 4."""
    return _conv_fwd(_CONV2D, x, weight, bias, relu)


def conv2d_bwd_data_f32(dy, dy_gate, weight, x_gate, x_shape):
    """dx of a 3x3 valid conv; dy zeroed where dy_gate <= 0, dx zeroed where x_gate <= 0 (either may be None)."""
    return _conv_bwd_data(_CONV2D, dy, dy_gate, weight, x_gate, x_shape)


def conv2d_bwd_weight_f32(x, dy, dy_gate, weight_shape):
    """(dw, dbias) of a 3x3 valid conv; deterministic (fixed slab split over images, slabs summed in order)."""
    return _conv_bwd_weight(_CONV2D, x, dy, dy_gate, weight_shape)


# ---- experiments/001_CNN_concat_all_timesteps_as_channels.py (csrc/conv2d_pool_f32.hip) ----
def conv2d144_sat_pool_fwd_f32(sat, x_coords, y_coords, weight, bias, n_frames):
    """relu(max_pool2d(conv2d(cat(frames 0..n_frames-1 of sat [B, T, H, W, 1], 5 synthesised channels), weight) + bias, 3))
    with x_coords [B, W], y_coords [B, H]; the input is built inside the kernel.  Returns (pooled [B, 144, (H-2)//3, (W-2)//3],
    codes uint8 of the same shape)."""
    who = "conv2d144_sat_pool_fwd_f32"
    b, t, h, w = _check_sat001(who, sat, x_coords, y_coords, n_frames)
    if tuple(weight.shape) != (C144, n_frames + 5, 3, 3):
        raise ValueError(f"{who}: weight [144, {n_frames + 5}, 3, 3] expected, got {tuple(weight.shape)}")
    if bias is None or tuple(bias.shape) != (C144,):
        raise ValueError(f"{who}: bias [144] expected")
    require_cuda(sat, x_coords, y_coords, weight, bias)
    _f32_contig(sat, x_coords, y_coords, weight, bias)
    y = torch.empty(_pooled_shape(b, C144, h, w), dtype=torch.float32, device=sat.device)
    codes = torch.empty(y.shape, dtype=torch.uint8, device=sat.device)
    check(getattr(get_lib(), "pv_" + who)(ptr(sat), ptr(x_coords), ptr(y_coords), ptr(weight), ptr(bias), ptr(y), ptr(codes),
                                          b, t, n_frames, h, w, C144, current_stream_ptr()), "pv_" + who)
    return y, codes


def conv2d144_sat_pool_bwd_weight_f32(sat, x_coords, y_coords, dy_pooled, codes, n_frames):
    """(dw [144, n_frames + 5, 3, 3], dbias) of conv2d144_sat_pool_fwd_f32, re-synthesising its input; deterministic."""
    who = "conv2d144_sat_pool_bwd_weight_f32"
    b, t, h, w = _check_sat001(who, sat, x_coords, y_coords, n_frames)
    _check_pooled(who, _CONV2D144_POOL, dy_pooled, codes, b, C144, h, w)
    require_cuda(sat, x_coords, y_coords, dy_pooled, codes)
    _f32_contig(sat, x_coords, y_coords, dy_pooled)
    _u8_contig(who, codes)
    ws, nbytes = _wgrad_ws("conv2d144", sat.device, b, n_frames + 5, C144, h, w, 1)
    dw, db = _grads_out((C144, n_frames + 5, 3, 3), C144, sat.device)
    check(getattr(get_lib(), "pv_" + who)(ptr(sat), ptr(x_coords), ptr(y_coords), ptr(dy_pooled), ptr(codes), ptr(dw),
                                          ptr(db), b, t, n_frames, h, w, C144, ptr(ws), nbytes, current_stream_ptr()),
                                          "pv_" + who)
    return dw, db


def conv2d144_fwd_f32(x, weight, bias, relu=True):
    """conv2d(x, weight) + bias (+ ReLU) for x [N, 144, H, W] -> [N, 144, H-2, W-2]."""
    return _conv_fwd(_CONV2D144, x, weight, bias, relu)


def conv2d144_bwd_data_f32(dy, dy_gate, weight, x_gate, x_shape):
    """dx of conv2d144_fwd_f32; dy zeroed where dy_gate <= 0, dx zeroed where x_gate <= 0 (either may be None)."""
    return _conv_bwd_data(_CONV2D144, dy, dy_gate, weight, x_gate, x_shape)


def conv2d144_bwd_weight_f32(x, dy, dy_gate, weight_shape):
    """(dw, dbias) of conv2d144_fwd_f32; deterministic (fixed slabs summed in order)."""
    return _conv_bwd_weight(_CONV2D144, x, dy, dy_gate, weight_shape)


def conv2d144_pool_fwd_f32(x, weight, bias):
    """relu(max_pool2d(conv2d(x, weight) + bias, 3)) for x [N, 144, H, W] -> (pooled, codes uint8)."""
    return _pool_fwd(_CONV2D144_POOL, x, weight, bias)


def conv2d144_pool_bwd_data_f32(dy_pooled, codes, weight, x_gate, x_shape):
    """dx of conv2d144_pool_fwd_f32 from the pooled gradient and the forward's codes; dx zeroed where x_gate <= 0."""
    return _pool_bwd_data(_CONV2D144_POOL, dy_pooled, codes, weight, x_gate, x_shape)


def conv2d144_pool_bwd_weight_f32(x, dy_pooled, codes, weight_shape):
    """(dw, dbias) of conv2d144_pool_fwd_f32 from the pooled gradient and the codes; deterministic."""
    return _pool_bwd_weight(_CONV2D144_POOL, x, dy_pooled, codes, weight_shape)


# ---- notebooks/16_maxpool.ipynb: Conv2d 6 -> 16 -> 32 -> 32 -> 32 (+ MaxPool2d(3)), ConvTranspose2d 32 -> 32 -> 16 -> 16 -> 1,
# cropped normalised MSE (csrc/conv2d_ae_f32.hip); planes up to 128 wide ----
def conv2d_ae_counts_fwd_f32(history, flow_pred, horizon, weight, bias):
    """relu(conv2d(cat(normalise(history), normalise(flow_pred)[:, None], horizon plane), weight) + bias): history
    [N, 4, H, W] and flow_pred [N, H, W] as int16 or f32 counts, horizon [N] f32 -> [N, 16, H-2, W-2]."""
    return _counts_fwd(_CONV2D_AE, history, flow_pred, horizon, weight, bias)


def conv2d_ae_counts_bwd_weight_f32(history, flow_pred, horizon, dy, weight_shape):
    """(dw [16, 6, 3, 3], dbias) of conv2d_ae_counts_fwd_f32's conv from its pre-activation gradient dy."""
    return _counts_bwd_weight(_CONV2D_AE, history, flow_pred, horizon, dy, weight_shape)


def _ae_family(padding):
    if padding not in (0, 2):
        raise ValueError(f"conv2d_ae: padding 0 or 2 expected, got {padding}")
    return _CONV2D_AE_P2 if padding else _CONV2D_AE


def conv2d_ae_fwd_f32(x, weight, bias, relu=True, padding=0):
    """conv2d(x, weight, padding=padding) + bias (+ ReLU), W <= 128: (C_in, C_out) = (16, 32) or (32, 32) at padding 0; (32, 32)
    at padding 2 (notebook 11's conv.4, pv_conv2d_ae_p2_*), W + 2 <= 128."""
    return _conv_fwd(_ae_family(padding), x, weight, bias, relu)


def conv2d_ae_bwd_data_f32(dy, dy_gate, weight, x_gate, x_shape, padding=0):
    """dx of conv2d_ae_fwd_f32; dy zeroed where dy_gate <= 0, dx zeroed where x_gate <= 0 (either may be None)."""
    return _conv_bwd_data(_ae_family(padding), dy, dy_gate, weight, x_gate, x_shape)


def conv2d_ae_bwd_weight_f32(x, dy, dy_gate, weight_shape, padding=0):
    """(dw, dbias) of conv2d_ae_fwd_f32; deterministic (fixed slabs summed in order)."""
    return _conv_bwd_weight(_ae_family(padding), x, dy, dy_gate, weight_shape)


def conv2d_ae_pool_fwd_f32(x, weight, bias):
    """relu(max_pool2d(conv2d(x, weight) + bias, 3)) for x [N, 32, H, W] -> (pooled, codes uint8)."""
    return _pool_fwd(_CONV2D_AE_POOL, x, weight, bias)


def conv2d_ae_pool_bwd_data_f32(dy_pooled, codes, weight, x_gate, x_shape):
    """dx of conv2d_ae_pool_fwd_f32 from the pooled gradient and the forward's codes; dx zeroed where x_gate <= 0."""
    return _pool_bwd_data(_CONV2D_AE_POOL, dy_pooled, codes, weight, x_gate, x_shape)


def conv2d_ae_pool_bwd_weight_f32(x, dy_pooled, codes, weight_shape):
    """(dw, dbias) of conv2d_ae_pool_fwd_f32 from the pooled gradient and the codes; deterministic."""
    return _pool_bwd_weight(_CONV2D_AE_POOL, x, dy_pooled, codes, weight_shape)


def convt2d_ae_fwd_f32(x, weight, bias, relu=True):
    """conv_transpose2d(x, weight) + bias (+ ReLU): x [N, C_in, H, W], weight [C_in, C_out, 3, 3] -> [N, C_out, H+2, W+2]."""
    return _conv_fwd(_CONVT2D_AE, x, weight, bias, relu)


def convt2d_ae_bwd_data_f32(dy, dy_gate, weight, x_gate, x_shape):
    """dx of convt2d_ae_fwd_f32; dy zeroed where dy_gate <= 0, dx zeroed where x_gate <= 0 (either may be None)."""
    return _conv_bwd_data(_CONVT2D_AE, dy, dy_gate, weight, x_gate, x_shape)


def convt2d_ae_bwd_weight_f32(x, dy, dy_gate, weight_shape):
    """(dw [C_in, C_out, 3, 3], dbias [C_out]) of convt2d_ae_fwd_f32; deterministic (fixed slabs summed in order)."""
    return _conv_bwd_weight(_CONVT2D_AE, x, dy, dy_gate, weight_shape)


def mse_crop_norm_f32(y_hat, target, need_grad=True):
    """mse_loss(y_hat, normalise(target)[..., 8:-8, 8:-8]) for y_hat [N, P, Q] f32 and target [N, P+16, Q+16] counts (int16
    or f32).  Returns (loss f32[1], dy_hat or None)."""
    return _mse_norm("mse_crop_norm", y_hat, target, (), need_grad)


# ---- notebooks/14_back_to_2d_conv_AE.ipynb, 15_int16.ipynb: Conv2d 6 -> 16 -> 32 -> 32 -> 32, ConvTranspose2d 32 -> 32 -> 16
# -> 1, all 3x3 stride 2 (csrc/conv2d_s2_f32.hip); planes up to 128 wide on the wide side ----
def conv2d_s2_counts_fwd_f32(history, flow_pred, horizon, weight, bias):
    """relu(conv2d(cat(normalise(history), normalise(flow_pred)[:, None], horizon plane), weight, stride=2) + bias): history
    [N, 4, H, W] and flow_pred [N, H, W] as int16 or f32 counts, horizon [N] f32 -> [N, 16, (H-3)//2+1, (W-3)//2+1]."""
    return _counts_fwd(_CONV2D_S2, history, flow_pred, horizon, weight, bias)


def conv2d_s2_counts_bwd_weight_f32(history, flow_pred, horizon, dy, weight_shape):
    """(dw [16, 6, 3, 3], dbias) of conv2d_s2_counts_fwd_f32's conv from its pre-activation gradient dy."""
    return _counts_bwd_weight(_CONV2D_S2, history, flow_pred, horizon, dy, weight_shape)


def conv2d_s2_fwd_f32(x, weight, bias, relu=True):
    """conv2d(x, weight, stride=2) + bias (+ ReLU) for (C_in, C_out) = (16, 32) or (32, 32), W <= 128."""
    return _conv_fwd(_CONV2D_S2, x, weight, bias, relu)


def conv2d_s2_bwd_data_f32(dy, dy_gate, weight, x_gate, x_shape):
    """dx of conv2d_s2_fwd_f32; dy zeroed where dy_gate <= 0, dx zeroed where x_gate <= 0 (either may be None).  The rows and
    columns of x the forward never reads get exactly 0."""
    return _conv_bwd_data(_CONV2D_S2, dy, dy_gate, weight, x_gate, x_shape)


def conv2d_s2_bwd_weight_f32(x, dy, dy_gate, weight_shape):
    """(dw, dbias) of conv2d_s2_fwd_f32; deterministic (fixed slabs summed in order)."""
    return _conv_bwd_weight(_CONV2D_S2, x, dy, dy_gate, weight_shape)


def convt2d_s2_fwd_f32(x, weight, bias, relu=True):
    """conv_transpose2d(x, weight, stride=2) + bias (+ ReLU): x [N, C_in, H, W], weight [C_in, C_out, 3, 3] -> [N, C_out,
    2H+1, 2W+1] for (C_in, C_out) = (32, 32), (32, 16) or (16, 1)."""
    return _conv_fwd(_CONVT2D_S2, x, weight, bias, relu)


def convt2d_s2_bwd_data_f32(dy, dy_gate, weight, x_gate, x_shape):
    """dx of convt2d_s2_fwd_f32; dy zeroed where dy_gate <= 0, dx zeroed where x_gate <= 0 (either may be None)."""
    return _conv_bwd_data(_CONVT2D_S2, dy, dy_gate, weight, x_gate, x_shape)


def convt2d_s2_bwd_weight_f32(x, dy, dy_gate, weight_shape):
    """(dw [C_in, C_out, 3, 3], dbias [C_out]) of convt2d_s2_fwd_f32; deterministic (fixed slabs summed in order)."""
    return _conv_bwd_weight(_CONVT2D_S2, x, dy, dy_gate, weight_shape)


# ---- notebooks/10_just_conv.ipynb: Conv2d 5 -> 64 -> 128 -> 128 (padding 2) -> 1 (stride 2, padding 2), the fifth input
# channel a forecast-horizon stripe (csrc/conv2d_wide_f32.hip); planes up to 128 wide ----
def _check_stripe(who, history, stripe_start, stripe_width):
    if history.dim() != 4 or not 1 <= history.shape[1] <= STRIPE_MAX_HIST:
        raise ValueError(f"{who}: history [N, 1..{STRIPE_MAX_HIST}, H, W] expected, got {tuple(history.shape)}")
    n, n_hist, h, w = history.shape
    if tuple(stripe_start.shape) != (n,) or stripe_start.dtype != torch.int32 or not stripe_start.is_contiguous():
        raise ValueError(f"{who}: stripe_start int32 [{n}] expected, got {stripe_start.dtype} {tuple(stripe_start.shape)}")
    if h < 3 or w < 3 or w > WIDE_MAX_W or stripe_width < 0:
        raise ValueError(f"{who}: planes of 3 x 3 up to {WIDE_MAX_W} columns and a stripe width >= 0 expected, got {h} x {w}, "
                         f"width {stripe_width}")
    require_cuda(history, stripe_start)
    _f32_contig(history)
    return n, n_hist, h, w


def _stripe_fwd(fam, history, stripe_start, weight, bias, stripe_width):
    """pv_{stem}_stripe_fwd_f32 on the family's output rule."""
    who = f"{fam.stem}_stripe_fwd_f32"
    n, n_hist, h, w = _check_stripe(who, history, stripe_start, stripe_width)
    if tuple(weight.shape) != (STRIPE_C_OUT, n_hist + 1, 3, 3):
        raise ValueError(f"{who}: weight [{STRIPE_C_OUT}, {n_hist + 1}, 3, 3] expected, got {tuple(weight.shape)}")
    if bias is None or tuple(bias.shape) != (STRIPE_C_OUT,):
        raise ValueError(f"{who}: bias [{STRIPE_C_OUT}] expected")
    require_cuda(weight, bias)
    _f32_contig(weight, bias)
    y = torch.empty((n, STRIPE_C_OUT, *fam.out_hw(h, w)), dtype=torch.float32, device=history.device)
    check(getattr(get_lib(), "pv_" + who)(ptr(history), ptr(stripe_start), ptr(weight), ptr(bias), ptr(y), n, n_hist, h, w,
                                          STRIPE_C_OUT, int(stripe_width), current_stream_ptr()), "pv_" + who)
    return y


def _stripe_bwd_weight(fam, history, stripe_start, dy, weight_shape, stripe_width):
    """pv_{stem}_stripe_bwd_weight_f32 on the family's output rule and weight-gradient workspace."""
    who = f"{fam.stem}_stripe_bwd_weight_f32"
    n, n_hist, h, w = _check_stripe(who, history, stripe_start, stripe_width)
    y_shape = (n, STRIPE_C_OUT, *fam.out_hw(h, w))
    if tuple(weight_shape) != (STRIPE_C_OUT, n_hist + 1, 3, 3) or tuple(dy.shape) != y_shape:
        raise ValueError(f"{who}: weight {(STRIPE_C_OUT, n_hist + 1, 3, 3)} and dy {y_shape} expected, got "
                         f"{tuple(weight_shape)} / {tuple(dy.shape)}")
    require_cuda(dy)
    _f32_contig(dy)
    ws, nbytes = _wgrad_ws(fam.stem, history.device, n, n_hist + 1, STRIPE_C_OUT, h, w, *fam.pad_args,
                            *fam.ws_args)
    dw, db = _grads_out(weight_shape, STRIPE_C_OUT, history.device)
    check(getattr(get_lib(), "pv_" + who)(ptr(history), ptr(stripe_start), ptr(dy), ptr(dw), ptr(db), n, n_hist, h, w,
                                          STRIPE_C_OUT, int(stripe_width), ptr(ws), nbytes, current_stream_ptr()),
          "pv_" + who)
    return dw, db


def conv2d_wide_stripe_fwd_f32(history, stripe_start, weight, bias, stripe_width):
    """relu(conv2d(cat(history, stripe plane), weight) + bias): history [N, n_hist, H, W] f32, the stripe plane of example i is 1
    on columns stripe_start[i] <= c < stripe_start[i] + stripe_width (inside the image) -> [N, 64, H - 2, W - 2]."""
    return _stripe_fwd(_CONV2D_WIDE_P0, history, stripe_start, weight, bias, stripe_width)


def conv2d_wide_stripe_bwd_weight_f32(history, stripe_start, dy, weight_shape, stripe_width):
    """(dw [64, n_hist + 1, 3, 3], dbias) of conv2d_wide_stripe_fwd_f32's conv from its pre-activation gradient dy."""
    return _stripe_bwd_weight(_CONV2D_WIDE_P0, history, stripe_start, dy, weight_shape, stripe_width)


def _wide_family(padding):
    if padding not in (0, 2):
        raise ValueError(f"conv2d_wide: padding 0 or 2 expected, got {padding}")
    return _CONV2D_WIDE_P2 if padding else _CONV2D_WIDE_P0


def conv2d_wide_fwd_f32(x, weight, bias, relu=True, padding=0):
    """conv2d(x, weight, padding=padding) + bias (+ ReLU) for (C_in, C_out) = (64, 128) or (128, 128), padding 0 or 2, W <= 128."""
    return _conv_fwd(_wide_family(padding), x, weight, bias, relu)


def conv2d_wide_bwd_data_f32(dy, dy_gate, weight, x_gate, x_shape, padding=0):
    """dx of conv2d_wide_fwd_f32; dy zeroed where dy_gate <= 0, dx zeroed where x_gate <= 0 (either may be None)."""
    return _conv_bwd_data(_wide_family(padding), dy, dy_gate, weight, x_gate, x_shape)


def conv2d_wide_bwd_weight_f32(x, dy, dy_gate, weight_shape, padding=0):
    """(dw, dbias) of conv2d_wide_fwd_f32; deterministic (fixed slabs summed in order)."""
    return _conv_bwd_weight(_wide_family(padding), x, dy, dy_gate, weight_shape)


# the padding-2 passes under the (forward, data gradient, weight gradient) signatures conv2d_functional.ConvReLU calls
def conv2d_wide_p2_fwd_f32(x, weight, bias, relu=True):
    return conv2d_wide_fwd_f32(x, weight, bias, relu, 2)


def conv2d_wide_p2_bwd_data_f32(dy, dy_gate, weight, x_gate, x_shape):
    return conv2d_wide_bwd_data_f32(dy, dy_gate, weight, x_gate, x_shape, 2)


def conv2d_wide_p2_bwd_weight_f32(x, dy, dy_gate, weight_shape):
    return conv2d_wide_bwd_weight_f32(x, dy, dy_gate, weight_shape, 2)


def conv2d_head_s2_fwd_f32(x, weight, bias, relu=False):
    """conv2d(x, weight [1, C_in, 3, 3], stride=2, padding=2) + bias (+ ReLU): [N, C_in, H, W] -> [N, 1, (H+1)//2+1, (W+1)//2+1]."""
    return _conv_fwd(_CONV2D_HEAD_S2, x, weight, bias, relu)


def conv2d_head_s2_bwd_data_f32(dy, dy_gate, weight, x_gate, x_shape):
    """dx of conv2d_head_s2_fwd_f32, zeroed where x_gate <= 0 (may be None); dy_gate must be None (no ReLU follows the head)."""
    return _conv_bwd_data(_CONV2D_HEAD_S2, dy, dy_gate, weight, x_gate, x_shape)


def conv2d_head_s2_bwd_weight_f32(x, dy, dy_gate, weight_shape):
    """(dw [1, C_in, 3, 3], dbias [1]) of conv2d_head_s2_fwd_f32; deterministic; dy_gate must be None."""
    return _conv_bwd_weight(_CONV2D_HEAD_S2, x, dy, dy_gate, weight_shape)


def mse_window_norm_f32(y_hat, target, row0=0, col0=0, need_grad=True):
    """mse_loss(y_hat, normalise(target)[..., row0:row0 + P, col0:col0 + Q]) for y_hat [N, P, Q] f32 and target [N, T, U]
    counts (int16 or f32).  Returns (loss f32[1], dy_hat or None)."""
    return _mse_norm("mse_window_norm", y_hat, target, (row0, col0), need_grad)


# ---- notebooks/09_horizon_represented_as_a_stripe.ipynb: Conv2d 5 -> 64 -> 128 -> 128 and ConvTranspose2d 128 -> 128 -> 128,
# all 3x3 stride 2, then ConvTranspose2d 128 -> 1 stride 1 (csrc/conv2d_wide_s2_f32.hip); planes up to 128 wide ----
def conv2d_wide_s2_stripe_fwd_f32(history, stripe_start, weight, bias, stripe_width):
    """relu(conv2d(cat(history, stripe plane), weight, stride=2) + bias) -> [N, 64, (H - 3) // 2 + 1, (W - 3) // 2 + 1]; the
    stripe plane as in conv2d_wide_stripe_fwd_f32."""
    return _stripe_fwd(_CONV2D_WIDE_S2, history, stripe_start, weight, bias, stripe_width)


def conv2d_wide_s2_stripe_bwd_weight_f32(history, stripe_start, dy, weight_shape, stripe_width):
    """(dw [64, n_hist + 1, 3, 3], dbias) of conv2d_wide_s2_stripe_fwd_f32's conv from its pre-activation gradient dy."""
    return _stripe_bwd_weight(_CONV2D_WIDE_S2, history, stripe_start, dy, weight_shape, stripe_width)


def conv2d_wide_s2_fwd_f32(x, weight, bias, relu=True):
    """conv2d(x, weight, stride=2) + bias (+ ReLU) for (C_in, C_out) = (64, 128) or (128, 128), W <= 128."""
    return _conv_fwd(_CONV2D_WIDE_S2, x, weight, bias, relu)


def conv2d_wide_s2_bwd_data_f32(dy, dy_gate, weight, x_gate, x_shape):
    """dx of conv2d_wide_s2_fwd_f32; dy zeroed where dy_gate <= 0, dx zeroed where x_gate <= 0 (either may be None).  The last
    row / column of an even-sized x, which the forward never reads, is exactly 0."""
    return _conv_bwd_data(_CONV2D_WIDE_S2, dy, dy_gate, weight, x_gate, x_shape)


def conv2d_wide_s2_bwd_weight_f32(x, dy, dy_gate, weight_shape):
    """(dw, dbias) of conv2d_wide_s2_fwd_f32; deterministic (fixed slabs summed in order)."""
    return _conv_bwd_weight(_CONV2D_WIDE_S2, x, dy, dy_gate, weight_shape)


def convt2d_wide_s2_fwd_f32(x, weight, bias, relu=True):
    """conv_transpose2d(x, weight [128, 128, 3, 3], stride=2) + bias (+ ReLU): [N, 128, H, W] -> [N, 128, 2H+1, 2W+1], 2W+1 <=
    128."""
    return _conv_fwd(_CONVT2D_WIDE_S2, x, weight, bias, relu)


def convt2d_wide_s2_bwd_data_f32(dy, dy_gate, weight, x_gate, x_shape):
    """dx of convt2d_wide_s2_fwd_f32; dy zeroed where dy_gate <= 0, dx zeroed where x_gate <= 0 (either may be None)."""
    return _conv_bwd_data(_CONVT2D_WIDE_S2, dy, dy_gate, weight, x_gate, x_shape)


def convt2d_wide_s2_bwd_weight_f32(x, dy, dy_gate, weight_shape):
    """(dw [128, 128, 3, 3], dbias) of convt2d_wide_s2_fwd_f32; deterministic."""
    return _conv_bwd_weight(_CONVT2D_WIDE_S2, x, dy, dy_gate, weight_shape)


def convt2d_head_fwd_f32(x, weight, bias, relu=False):
    """conv_transpose2d(x, weight [C_in, 1, 3, 3]) + bias (+ ReLU): [N, C_in, H, W] -> [N, 1, H + 2, W + 2], W <= 128."""
    return _conv_fwd(_CONVT2D_HEAD, x, weight, bias, relu)


def convt2d_head_bwd_data_f32(dy, dy_gate, weight, x_gate, x_shape):
    """dx of convt2d_head_fwd_f32, zeroed where x_gate <= 0 (may be None); dy_gate must be None (no ReLU follows the head)."""
    return _conv_bwd_data(_CONVT2D_HEAD, dy, dy_gate, weight, x_gate, x_shape)


def convt2d_head_bwd_weight_f32(x, dy, dy_gate, weight_shape):
    """(dw [C_in, 1, 3, 3], dbias [1]) of convt2d_head_fwd_f32; deterministic; dy_gate must be None."""
    return _conv_bwd_weight(_CONVT2D_HEAD, x, dy, dy_gate, weight_shape)


def mse_pred_window_f32(y_hat, target, row0=0, col0=0, need_grad=True):
    """mse_loss(y_hat[..., row0:row0 + T, col0:col0 + U], target) for y_hat [N, P, Q] and target [N, T, U], both f32.  Returns
    (loss f32[1], dy_hat or None); dy_hat covers all of y_hat and is exactly 0 outside the window."""
    who = "mse_pred_window_f32"
    if not (y_hat.dim() == 3 and target.dim() == 3 and target.shape[0] == y_hat.shape[0]):
        raise ValueError(f"{who}: y_hat [N, P, Q] and target [N, T, U] expected, got {tuple(y_hat.shape)} / "
                         f"{tuple(target.shape)}")
    require_cuda(y_hat, target)
    _f32_contig(y_hat, target)
    n, oh, ow = y_hat.shape
    loss = torch.empty((1,), dtype=torch.float32, device=y_hat.device)
    grad = torch.empty_like(y_hat) if need_grad else None
    ws = _workspace("mse_pred_window", 4 * n, y_hat.device)
    check(get_lib().pv_mse_pred_window_f32(ptr(y_hat), ptr(target), n, oh, ow, target.shape[1], target.shape[2], int(row0),
                                           int(col0), ptr(loss), ptr(grad), ptr(ws), 4 * n, current_stream_ptr()),
          "pv_" + who)
    return loss, grad


# ---- notebooks/12_just_3d_conv.ipynb: Conv3d 2 -> 64 -> 128 -> 128 -> 128 -> 1, kernel (2, 3, 3), spatial padding 1, the
# second input channel the forecast horizon (csrc/conv3d_wide_f32.hip); planes up to 128 wide.  A 3-D family is a _ConvFamily
# record whose shape rule is written out (_check_conv3d_wide); its passes are _conv_fwd, _conv_bwd_data, _conv_bwd_weight. ----
HORIZON_C_OUT = 64


def head_s2p1_out(side):
    """Side of a 3x3 stride-2 padding-1 Conv2d's output."""
    return (side - 1) // 2 + 1


_CONV2D_HEAD_S2P1 = _conv2d_family("conv2d_head_s2p1", lambda *a: _check_head(*a),
                                   lambda h, w: (head_s2p1_out(h), head_s2p1_out(w)))


def _check_conv3d_wide(who, x_shape, weight_shape, padding):
    """The shape rule of pv_conv3d_wide_*: x [N, C_in, D, H, W], weight [C_out, C_in, 2, 3, 3], padding (0 | 1, 1, 1).
    Returns the entry points' (n, c_in, c_out, d, h, w, pad_d, pad_hw) and the output's shape."""
    if not (len(x_shape) == 5 and len(weight_shape) == 5 and tuple(weight_shape[1:]) == (x_shape[1], 2, 3, 3)):
        raise ValueError(f"{who}: x [N, C_in, D, H, W] and weight [C_out, C_in, 2, 3, 3] expected, got {tuple(x_shape)} / "
                         f"{tuple(weight_shape)}")
    n, ci, d, h, w = (int(v) for v in x_shape)
    co = int(weight_shape[0])
    if (ci, co) not in WIDE_PAIRS:
        raise ValueError(f"{who}: (C_in, C_out) = (64, 128) or (128, 128) expected, got ({ci}, {co})")
    padding = tuple(int(p) for p in padding)
    if len(padding) != 3 or padding[0] not in (0, 1) or padding[1:] != (1, 1):
        raise ValueError(f"{who}: padding (0, 1, 1) or (1, 1, 1) expected, got {padding}")
    d_out = d + 2 * padding[0] - 1
    if d_out < 1 or min(h, w) < 1 or w > WIDE_MAX_W:
        raise ValueError(f"{who}: an output of at least one slice and planes of 1 to {WIDE_MAX_W} columns expected, got "
                         f"{tuple(x_shape)} with padding {padding}")
    return (n, ci, co, d, h, w, padding[0], 1), (n, co, d_out, h, w)


def _conv3d_wide(padding):
    return _ConvFamily("conv3d_wide", lambda who, x_shape, w_shape: _check_conv3d_wide(who, x_shape, w_shape, padding))


def conv3d_wide_fwd_f32(x, weight, bias, relu=True, padding=(0, 1, 1)):
    """conv3d(x, weight, stride 1, padding (0 | 1, 1, 1)) + bias (+ ReLU): [N, 64 | 128, D, H, W] f32 -> [N, 128, D + 2 pd - 1,
    H, W]; weight [128, C_in, 2, 3, 3]."""
    return _conv_fwd(_conv3d_wide(padding), x, weight, bias, relu)


def conv3d_wide_bwd_data_f32(dy, dy_gate, weight, x_gate, x_shape, padding=(0, 1, 1)):
    """dx of conv3d_wide_fwd_f32; dy zeroed where dy_gate <= 0, dx zeroed where x_gate <= 0 (either may be None)."""
    return _conv_bwd_data(_conv3d_wide(padding), dy, dy_gate, weight, x_gate, x_shape)


def conv3d_wide_bwd_weight_f32(x, dy, dy_gate, weight_shape, padding=(0, 1, 1)):
    """(dw, dbias) of conv3d_wide_fwd_f32; deterministic (fixed slabs summed in order)."""
    return _conv_bwd_weight(_conv3d_wide(padding), x, dy, dy_gate, weight_shape)


def _check_horizon(who, history, horizon, weight_shape):
    if history.dim() != 4 or history.shape[1] < 2:
        raise ValueError(f"{who}: history [N, D >= 2, H, W] expected, got {tuple(history.shape)}")
    n, d, h, w = (int(v) for v in history.shape)
    if tuple(horizon.shape) != (n,):
        raise ValueError(f"{who}: horizon [{n}] expected, got {tuple(horizon.shape)}")
    if tuple(weight_shape) != (HORIZON_C_OUT, 2, 2, 3, 3):
        raise ValueError(f"{who}: weight [{HORIZON_C_OUT}, 2, 2, 3, 3] expected, got {tuple(weight_shape)}")
    if min(h, w) < 1 or w > WIDE_MAX_W:
        raise ValueError(f"{who}: planes of 1 to {WIDE_MAX_W} columns expected, got {h} x {w}")
    require_cuda(history, horizon)
    _f32_contig(history, horizon)
    return n, d, h, w


def conv3d_wide_horizon_fwd_f32(history, horizon, weight, bias):
    """relu(conv3d(cat(history.unsqueeze(1), horizon plane), weight, padding (0, 1, 1)) + bias): history [N, D, H, W] f32, the
    second input channel of example i is horizon[i] everywhere inside the image -> [N, 64, D - 1, H, W]."""
    who = "conv3d_wide_horizon_fwd_f32"
    n, d, h, w = _check_horizon(who, history, horizon, weight.shape)
    if bias is None or tuple(bias.shape) != (HORIZON_C_OUT,):
        raise ValueError(f"{who}: bias [{HORIZON_C_OUT}] expected")
    require_cuda(weight, bias)
    _f32_contig(weight, bias)
    y = torch.empty((n, HORIZON_C_OUT, d - 1, h, w), dtype=torch.float32, device=history.device)
    check(get_lib().pv_conv3d_wide_horizon_fwd_f32(ptr(history), ptr(horizon), ptr(weight), ptr(bias), ptr(y), n, d, h, w,
                                                   HORIZON_C_OUT, current_stream_ptr()), "pv_" + who)
    return y


def conv3d_wide_horizon_bwd_weight_f32(history, horizon, dy, weight_shape):
    """(dw [64, 2, 2, 3, 3], dbias) of conv3d_wide_horizon_fwd_f32's conv from its pre-activation gradient dy."""
    who = "conv3d_wide_horizon_bwd_weight_f32"
    n, d, h, w = _check_horizon(who, history, horizon, weight_shape)
    y_shape = (n, HORIZON_C_OUT, d - 1, h, w)
    if tuple(dy.shape) != y_shape:
        raise ValueError(f"{who}: dy {y_shape} expected, got {tuple(dy.shape)}")
    require_cuda(dy)
    _f32_contig(dy)
    ws, nbytes = _wgrad_ws("conv3d_wide_horizon", history.device, n, d, h, w, HORIZON_C_OUT)
    dw, db = _grads_out(weight_shape, HORIZON_C_OUT, history.device)
    check(get_lib().pv_conv3d_wide_horizon_bwd_weight_f32(ptr(history), ptr(horizon), ptr(dy), ptr(dw), ptr(db), n, d, h, w,
                                                          HORIZON_C_OUT, ptr(ws), nbytes, current_stream_ptr()), "pv_" + who)
    return dw, db


def conv2d_head_s2p1_fwd_f32(x, weight, bias, relu=False):
    """conv2d(x, weight, stride 2, padding 1) + bias (+ ReLU): [N, C_in, H, W] f32 -> [N, 1, (H - 1) // 2 + 1, (W - 1) // 2 + 1]."""
    return _conv_fwd(_CONV2D_HEAD_S2P1, x, weight, bias, relu)


def conv2d_head_s2p1_bwd_data_f32(dy, dy_gate, weight, x_gate, x_shape):
    """dx of conv2d_head_s2p1_fwd_f32, zeroed where x_gate <= 0 (may be None); dy_gate must be None (no ReLU follows the head)."""
    return _conv_bwd_data(_CONV2D_HEAD_S2P1, dy, dy_gate, weight, x_gate, x_shape)


def conv2d_head_s2p1_bwd_weight_f32(x, dy, dy_gate, weight_shape):
    """(dw [1, C_in, 3, 3], dbias [1]) of conv2d_head_s2p1_fwd_f32; deterministic; dy_gate must be None."""
    return _conv_bwd_weight(_CONV2D_HEAD_S2P1, x, dy, dy_gate, weight_shape)


def _head_d2_views(who, x_shape, weight_shape):
    """conv3d(x, weight, stride (1, 2, 2), padding (0, 1, 1)) with weight [1, C, 2, 3, 3] on an input of depth 2 is the 3x3
    stride-2 padding-1 Conv2d on x [N, 2 C, H, W] and weight [1, 2 C, 3, 3]: both are views (depth is the axis after the
    channels).  Any other depth is refused."""
    if not (len(x_shape) == 5 and len(weight_shape) == 5 and tuple(weight_shape) == (1, x_shape[1], 2, 3, 3)):
        raise ValueError(f"{who}: x [N, C, 2, H, W] and weight [1, C, 2, 3, 3] expected, got {tuple(x_shape)} / "
                         f"{tuple(weight_shape)}")
    n, c, d, h, w = (int(v) for v in x_shape)
    if d != 2:
        raise ValueError(f"{who}: an input of depth 2 expected (one output slice), got depth {d}")
    return (n, 2 * c, h, w), (1, 2 * c, 3, 3)


def conv3d_head_d2_fwd_f32(x, weight, bias, relu=False):
    """conv3d(x [N, C, 2, H, W], weight [1, C, 2, 3, 3], stride (1, 2, 2), padding (0, 1, 1)) + bias -> [N, 1, 1, H', W']."""
    x2, w2 = _head_d2_views("conv3d_head_d2_fwd_f32", x.shape, weight.shape)
    _f32_contig(x, weight)
    return conv2d_head_s2p1_fwd_f32(x.view(x2), weight.view(w2), bias, relu).unsqueeze(2)


def conv3d_head_d2_bwd_data_f32(dy, dy_gate, weight, x_gate, x_shape):
    """dx [N, C, 2, H, W] of conv3d_head_d2_fwd_f32 from dy [N, 1, 1, H', W'], zeroed where x_gate <= 0; dy_gate must be None."""
    x2, w2 = _head_d2_views("conv3d_head_d2_bwd_data_f32", x_shape, weight.shape)
    _f32_contig(dy, weight, x_gate)
    if dy.dim() != 5 or dy.shape[2] != 1:
        raise ValueError(f"conv3d_head_d2_bwd_data_f32: dy [N, 1, 1, H', W'] expected, got {tuple(dy.shape)}")
    dx = conv2d_head_s2p1_bwd_data_f32(dy.squeeze(2), dy_gate, weight.view(w2), None if x_gate is None else x_gate.view(x2), x2)
    return dx.view(tuple(x_shape))


def conv3d_head_d2_bwd_weight_f32(x, dy, dy_gate, weight_shape):
    """(dw [1, C, 2, 3, 3], dbias [1]) of conv3d_head_d2_fwd_f32; deterministic; dy_gate must be None."""
    x2, w2 = _head_d2_views("conv3d_head_d2_bwd_weight_f32", x.shape, weight_shape)
    _f32_contig(x, dy)
    if dy.dim() != 5 or dy.shape[2] != 1:
        raise ValueError(f"conv3d_head_d2_bwd_weight_f32: dy [N, 1, 1, H', W'] expected, got {tuple(dy.shape)}")
    dw, db = conv2d_head_s2p1_bwd_weight_f32(x.view(x2), dy.squeeze(2), dy_gate, w2)
    return dw.view(tuple(weight_shape)), db


# ---- notebooks/08_multiple_historical_images_as_separate_channels.ipynb: Conv3d 1 -> 8 -> 32 -> 32, kernel (2, 3, 3), stride
# (1, 2, 2), no padding, then ConvTranspose2d 33 -> 32 whose last input channel is the forecast horizon
# (csrc/conv3d_s2_f32.hip); planes up to 128 wide.  The family's shape rule is _check_conv3d_s2. ----
CONV3D_S2_PAIRS = ((1, 8), (8, 32), (32, 32))     # (c_in, c_out) of pv_conv3d_s2_*
CONVT_HORIZON_C = 32                              # real input channels = output channels of pv_convt2d_s2_horizon_*


def _check_conv3d_s2(who, x_shape, weight_shape):
    """The shape rule of pv_conv3d_s2_*: x [N, C_in, D, H, W], weight [C_out, C_in, 2, 3, 3].  Returns the entry points' (n,
    c_in, c_out, d, h, w) and the output's shape."""
    if not (len(x_shape) == 5 and len(weight_shape) == 5 and tuple(weight_shape[1:]) == (x_shape[1], 2, 3, 3)):
        raise ValueError(f"{who}: x [N, C_in, D, H, W] and weight [C_out, C_in, 2, 3, 3] expected, got {tuple(x_shape)} / "
                         f"{tuple(weight_shape)}")
    n, ci, d, h, w = (int(v) for v in x_shape)
    co = int(weight_shape[0])
    if (ci, co) not in CONV3D_S2_PAIRS:
        raise ValueError(f"{who}: (C_in, C_out) = (1, 8), (8, 32) or (32, 32) expected, got ({ci}, {co})")
    if d < 2 or min(h, w) < 3 or w > WIDE_MAX_W:
        raise ValueError(f"{who}: at least two slices and planes of 3 to {WIDE_MAX_W} columns expected, got {tuple(x_shape)}")
    return (n, ci, co, d, h, w), (n, co, d - 1, s2_out(h), s2_out(w))


def _check_conv3d_s2_dgrad(who, x_shape, weight_shape):
    dims, y_shape = _check_conv3d_s2(who, x_shape, weight_shape)
    if dims[1] == 1:
        raise ValueError(f"{who}: the (1, 8) layer is the first one and has no data gradient")
    return dims, y_shape


_CONV3D_S2 = _ConvFamily("conv3d_s2", _check_conv3d_s2)


def conv3d_s2_fwd_f32(x, weight, bias, relu=True):
    """conv3d(x, weight, stride (1, 2, 2)) + bias (+ ReLU): [N, C_in, D, H, W] f32 -> [N, C_out, D - 1, (H - 3) // 2 + 1, (W - 3)
    // 2 + 1]; weight [C_out, C_in, 2, 3, 3]."""
    return _conv_fwd(_CONV3D_S2, x, weight, bias, relu)


def conv3d_s2_bwd_data_f32(dy, dy_gate, weight, x_gate, x_shape):
    """dx of conv3d_s2_fwd_f32; dy zeroed where dy_gate <= 0, dx zeroed where x_gate <= 0 (either may be None).  The rows and
    columns of x the forward never reads are written as 0.  The 1 -> 8 layer has no data gradient."""
    return _conv_bwd_data(_CONV3D_S2._replace(shape=_check_conv3d_s2_dgrad), dy, dy_gate, weight, x_gate, x_shape)


def conv3d_s2_bwd_weight_f32(x, dy, dy_gate, weight_shape):
    """(dw, dbias) of conv3d_s2_fwd_f32; deterministic (fixed slabs summed in order)."""
    return _conv_bwd_weight(_CONV3D_S2, x, dy, dy_gate, weight_shape)


def _check_convt_horizon(who, x, horizon, weight_shape, out_hw):
    """The shape rule of pv_convt2d_{s2,ae}_horizon_*; out_hw(h, w) = the output's sides.  Returns (n, h, w) and the output's
    shape."""
    c = CONVT_HORIZON_C
    if x.dim() != 4 or x.shape[1] != c or tuple(weight_shape) != (c + 1, c, 3, 3):
        raise ValueError(f"{who}: x [N, {c}, H, W] and weight [{c + 1}, {c}, 3, 3] expected, got {tuple(x.shape)} / "
                         f"{tuple(weight_shape)}")
    n, _, h, w = (int(v) for v in x.shape)
    if tuple(horizon.shape) != (n,):
        raise ValueError(f"{who}: horizon [{n}] expected, got {tuple(horizon.shape)}")
    if min(h, w) < 1 or out_hw(h, w)[1] > WIDE_MAX_W:
        raise ValueError(f"{who}: a non-empty plane whose output is at most {WIDE_MAX_W} columns wide expected, got {h} x {w}")
    return (n, h, w), (n, c, *out_hw(h, w))


def _convt_horizon_fwd(stem, out_hw, x, horizon, weight, bias, relu):
    who = f"{stem}_horizon_fwd_f32"
    dims, y_shape = _check_convt_horizon(who, x, horizon, weight.shape, out_hw)
    _check_bias(who, bias, CONVT_HORIZON_C)
    require_cuda(x, horizon, weight, bias)
    _f32_contig(x, horizon, weight, bias)
    y = torch.empty(y_shape, dtype=torch.float32, device=x.device)
    check(getattr(get_lib(), "pv_" + who)(ptr(x), ptr(horizon), ptr(weight), ptr(bias), ptr(y), *dims, int(relu),
                                          current_stream_ptr()), "pv_" + who)
    return y


def _convt_horizon_bwd_weight(stem, out_hw, x, horizon, dy, dy_gate, weight_shape):
    who = f"{stem}_horizon_bwd_weight_f32"
    dims, y_shape = _check_convt_horizon(who, x, horizon, weight_shape, out_hw)
    _check_dy(who, dy, dy_gate, y_shape)
    require_cuda(x, horizon, dy, dy_gate)
    _f32_contig(x, horizon, dy, dy_gate)
    ws, nbytes = _wgrad_ws(f"{stem}_horizon", x.device, *dims)
    dw, db = _grads_out(weight_shape, CONVT_HORIZON_C, x.device)
    check(getattr(get_lib(), "pv_" + who)(ptr(x), ptr(horizon), ptr(dy), ptr(dy_gate), ptr(dw), ptr(db), *dims, ptr(ws), nbytes,
                                          current_stream_ptr()), "pv_" + who)
    return dw, db


def _s2t_hw(h, w):
    return 2 * h + 1, 2 * w + 1


def convt2d_s2_horizon_fwd_f32(x, horizon, weight, bias, relu=True):
    """conv_transpose2d(cat(x, horizon plane), weight, stride 2) + bias (+ ReLU): x [N, 32, H, W] f32, input channel 32 of
    example i is horizon[i] everywhere -> [N, 32, 2 H + 1, 2 W + 1]; weight [33, 32, 3, 3]."""
    return _convt_horizon_fwd("convt2d_s2", _s2t_hw, x, horizon, weight, bias, relu)


def convt2d_s2_horizon_bwd_weight_f32(x, horizon, dy, dy_gate, weight_shape):
    """(dw [33, 32, 3, 3], dbias [32]) of convt2d_s2_horizon_fwd_f32; dy zeroed where dy_gate <= 0 (may be None);
    deterministic.  The data gradient of the 32 real channels is convt2d_s2_bwd_data_f32 on weight[:32]."""
    return _convt_horizon_bwd_weight("convt2d_s2", _s2t_hw, x, horizon, dy, dy_gate, weight_shape)


# ---- notebooks/05_more_image_inputs.ipynb: Conv2d 4 -> 32 whose four input channels are three tensors read in place, and
# ConvTranspose2d 33 -> 32 at stride 1 whose last input channel is the forecast horizon (csrc/conv2d_inputs_f32.hip); planes
# up to 128 wide.  The layers between them are conv2d_ae_*, convt2d_ae_* and convt2d_head_*. ----
INPUTS_C_OUT = 32                                 # CHANNELS


def _full_hw(h, w):
    return h + 2, w + 2


def _check_inputs4(who, flow_pred, t0, flow_field, weight_shape):
    if flow_pred.dim() != 3 or tuple(t0.shape) != tuple(flow_pred.shape):
        raise ValueError(f"{who}: flow prediction and t0 image [N, H, W] expected, got {tuple(flow_pred.shape)} / "
                         f"{tuple(t0.shape)}")
    n, h, w = (int(v) for v in flow_pred.shape)
    if tuple(flow_field.shape) != (n, 2, h, w) or tuple(weight_shape) != (INPUTS_C_OUT, 4, 3, 3):
        raise ValueError(f"{who}: flow field [{n}, 2, {h}, {w}] and weight [{INPUTS_C_OUT}, 4, 3, 3] expected, got "
                         f"{tuple(flow_field.shape)} / {tuple(weight_shape)}")
    require_cuda(flow_pred, t0, flow_field)
    _f32_contig(flow_pred, t0, flow_field)
    return n, h, w


def conv2d_ae_inputs_fwd_f32(flow_pred, t0, flow_field, weight, bias, relu=True):
    """conv2d(cat(flow_pred, t0, flow_field), weight) + bias (+ ReLU): flow prediction and t0 image [N, H, W], flow field
    [N, 2, H, W] (x then y), all f32 and read in place as input channels 0, 1 and 2 - 3 -> [N, 32, H - 2, W - 2]; weight
    [32, 4, 3, 3]; H, W >= 3, W <= 128."""
    who = "conv2d_ae_inputs_fwd_f32"
    n, h, w = _check_inputs4(who, flow_pred, t0, flow_field, weight.shape)
    _check_bias(who, bias, INPUTS_C_OUT)
    require_cuda(weight, bias)
    _f32_contig(weight, bias)
    # clamped: an undersized plane reaches the entry point, which names the smallest it takes
    y = torch.empty((n, INPUTS_C_OUT, max(h - 2, 0), max(w - 2, 0)), dtype=torch.float32, device=flow_pred.device)
    check(get_lib().pv_conv2d_ae_inputs_fwd_f32(ptr(flow_pred), ptr(t0), ptr(flow_field), ptr(weight), ptr(bias), ptr(y), n, h,
                                                w, int(relu), current_stream_ptr()), "pv_" + who)
    return y


def conv2d_ae_inputs_bwd_weight_f32(flow_pred, t0, flow_field, dy, weight_shape, dy_gate=None):
    """(dw [32, 4, 3, 3], dbias [32]) of conv2d_ae_inputs_fwd_f32; dy zeroed where dy_gate <= 0 (may be None); deterministic.
    The inputs are data, so there is no data gradient."""
    who = "conv2d_ae_inputs_bwd_weight_f32"
    n, h, w = _check_inputs4(who, flow_pred, t0, flow_field, weight_shape)
    _check_dy(who, dy, dy_gate, (n, INPUTS_C_OUT, h - 2, w - 2))
    require_cuda(dy, dy_gate)
    _f32_contig(dy, dy_gate)
    ws, nbytes = _wgrad_ws("conv2d_ae_inputs", flow_pred.device, n, h, w)
    dw, db = _grads_out(weight_shape, INPUTS_C_OUT, flow_pred.device)
    check(get_lib().pv_conv2d_ae_inputs_bwd_weight_f32(ptr(flow_pred), ptr(t0), ptr(flow_field), ptr(dy), ptr(dy_gate), ptr(dw),
                                                       ptr(db), n, h, w, ptr(ws), nbytes, current_stream_ptr()), "pv_" + who)
    return dw, db


def convt2d_ae_horizon_fwd_f32(x, horizon, weight, bias, relu=True):
    """conv_transpose2d(cat(x, horizon plane), weight) + bias (+ ReLU): x [N, 32, H, W] f32, input channel 32 of example i is
    horizon[i] everywhere -> [N, 32, H + 2, W + 2]; weight [33, 32, 3, 3]; W + 2 <= 128."""
    return _convt_horizon_fwd("convt2d_ae", _full_hw, x, horizon, weight, bias, relu)


def convt2d_ae_horizon_bwd_weight_f32(x, horizon, dy, dy_gate, weight_shape):
    """(dw [33, 32, 3, 3], dbias [32]) of convt2d_ae_horizon_fwd_f32; dy zeroed where dy_gate <= 0 (may be None);
    deterministic.  The data gradient of the 32 real channels is convt2d_ae_bwd_data_f32 on weight[:32]."""
    return _convt_horizon_bwd_weight("convt2d_ae", _full_hw, x, horizon, dy, dy_gate, weight_shape)


# ---- notebooks/07_multiple_historical_images.ipynb: one Conv2d 2 -> 32 -> 32 -> 32 stride-2 encoder applied to every history
# frame with the same weights (the frames folded into the batch, image FRAMES b + f), then ConvTranspose2d 128 -> 32 over the
# concatenated encoder outputs (csrc/conv2d_frames_f32.hip); planes up to 128 wide.  Layers 2 and 3 are conv2d_s2_* on
# [FRAMES B, 32, ..].  The shape rules are _check_frame_horizon and _check_convt_frames. ----
FRAME_C = 32                                      # CHANNELS: the encoder's width, per frame
HIST_FRAMES = 4                                   # N_HIST_IMAGES
CONVT_FRAMES_PAIR = (HIST_FRAMES * FRAME_C, FRAME_C)      # (c_in, c_out) of pv_convt2d_s2_frames_*


def _check_frame_horizon(who, history, horizon, weight_shape):
    """The shape rule of pv_conv2d_s2_frame_horizon_*: history [N, F, H, W], horizon [N], weight [32, 2, 3, 3].  Returns the
    entry points' (n, frames, h, w) and the output's shape."""
    if history.dim() != 4 or history.shape[1] < 1:
        raise ValueError(f"{who}: history [N, F >= 1, H, W] expected, got {tuple(history.shape)}")
    n, frames, h, w = (int(v) for v in history.shape)
    if tuple(horizon.shape) != (n,):
        raise ValueError(f"{who}: horizon [{n}] expected, got {tuple(horizon.shape)}")
    if tuple(weight_shape) != (FRAME_C, 2, 3, 3):
        raise ValueError(f"{who}: weight [{FRAME_C}, 2, 3, 3] expected, got {tuple(weight_shape)}")
    if min(h, w) < 3 or w > WIDE_MAX_W:
        raise ValueError(f"{who}: planes of 3 to {WIDE_MAX_W} columns expected, got {h} x {w}")
    return (n, frames, h, w), (n * frames, FRAME_C, s2_out(h), s2_out(w))


def conv2d_s2_frame_horizon_fwd_f32(history, horizon, weight, bias, relu=True):
    """conv2d(cat(history[:, f:f + 1], horizon plane), weight, stride 2) + bias (+ ReLU) for every frame f at once: history [N,
    F, H, W] f32 read in place, the second input channel of example i is horizon[i] everywhere -> [N F, 32, (H - 3) // 2 + 1,
    (W - 3) // 2 + 1] with image index F i + f; weight [32, 2, 3, 3]."""
    who = "conv2d_s2_frame_horizon_fwd_f32"
    dims, y_shape = _check_frame_horizon(who, history, horizon, weight.shape)
    _check_bias(who, bias, FRAME_C)
    require_cuda(history, horizon, weight, bias)
    _f32_contig(history, horizon, weight, bias)
    y = torch.empty(y_shape, dtype=torch.float32, device=history.device)
    check(get_lib().pv_conv2d_s2_frame_horizon_fwd_f32(ptr(history), ptr(horizon), ptr(weight), ptr(bias), ptr(y), *dims,
                                                       int(relu), current_stream_ptr()), "pv_" + who)
    return y


def conv2d_s2_frame_horizon_bwd_weight_f32(history, horizon, dy, weight_shape, dy_gate=None):
    """(dw [32, 2, 3, 3], dbias [32]) of conv2d_s2_frame_horizon_fwd_f32's conv, summed over its frames, from dy [N F, 32, ..]
    zeroed where dy_gate <= 0 (may be None); deterministic."""
    who = "conv2d_s2_frame_horizon_bwd_weight_f32"
    dims, y_shape = _check_frame_horizon(who, history, horizon, weight_shape)
    _check_dy(who, dy, dy_gate, y_shape)
    require_cuda(history, horizon, dy, dy_gate)
    _f32_contig(history, horizon, dy, dy_gate)
    ws, nbytes = _wgrad_ws("conv2d_s2_frame_horizon", history.device, *dims)
    dw, db = _grads_out(weight_shape, FRAME_C, history.device)
    check(get_lib().pv_conv2d_s2_frame_horizon_bwd_weight_f32(ptr(history), ptr(horizon), ptr(dy), ptr(dy_gate), ptr(dw),
                                                              ptr(db), *dims, ptr(ws), nbytes, current_stream_ptr()),
          "pv_" + who)
    return dw, db


def _check_convt_frames(who, x_shape, weight_shape):
    """The shape rule of pv_convt2d_s2_frames_*: x [N, 128, H, W], weight [128, 32, 3, 3]."""
    ci, co = CONVT_FRAMES_PAIR
    if not (len(x_shape) == 4 and x_shape[1] == ci and tuple(weight_shape) == (ci, co, 3, 3)):
        raise ValueError(f"{who}: x [N, {ci}, H, W] and weight [{ci}, {co}, 3, 3] expected, got {tuple(x_shape)} / "
                         f"{tuple(weight_shape)}")
    if min(x_shape[2:]) < 1 or 2 * x_shape[3] + 1 > WIDE_MAX_W:
        raise ValueError(f"{who}: a non-empty plane whose output is at most {WIDE_MAX_W} columns wide expected, got "
                         f"{x_shape[2]} x {x_shape[3]}")


_CONVT2D_S2_FRAMES = _conv2d_family("convt2d_s2_frames", _check_convt_frames, lambda h, w: (2 * h + 1, 2 * w + 1), c_out_axis=1)


def convt2d_s2_frames_fwd_f32(x, weight, bias, relu=True):
    """conv_transpose2d(x, weight, stride 2) + bias (+ ReLU): [N, 128, H, W] f32 -> [N, 32, 2 H + 1, 2 W + 1], 2 W + 1 <= 128;
    weight [128, 32, 3, 3]."""
    return _conv_fwd(_CONVT2D_S2_FRAMES, x, weight, bias, relu)


def convt2d_s2_frames_bwd_data_f32(dy, dy_gate, weight, x_gate, x_shape):
    """dx of convt2d_s2_frames_fwd_f32; dy zeroed where dy_gate <= 0, dx zeroed where x_gate <= 0 (either may be None)."""
    return _conv_bwd_data(_CONVT2D_S2_FRAMES, dy, dy_gate, weight, x_gate, x_shape)


def convt2d_s2_frames_bwd_weight_f32(x, dy, dy_gate, weight_shape):
    """(dw [128, 32, 3, 3], dbias [32]) of convt2d_s2_frames_fwd_f32; deterministic (fixed slabs summed in order)."""
    return _conv_bwd_weight(_CONVT2D_S2_FRAMES, x, dy, dy_gate, weight_shape)


# ---- notebooks/11_just_conv_and_conv_over_time.ipynb: Conv2d 2 -> 16 -> 32 -> 32 (padding 2) -> 1 (stride 2, padding 2) with a
# ReLU after each, applied to every history frame with the same weights and the forecast-horizon stripe as the second channel
# (the frames folded into the batch, image FRAMES b + f), then three (1, 2) convolutions over the four results per pixel
# (csrc/conv2d_ae_f32.hip, csrc/conv_time_f32.hip); planes up to 128 wide.  Layer 2 is conv2d_ae_*, layer 3 conv2d_ae_*(padding
# = 2), layer 4 conv2d_head_s2_* on [FRAMES B, 32, ..]. ----
FRAME_STRIPE_C_OUT = 16                           # CHANNELS // 2
TIME_FRAMES, TIME_C = 4, 16                       # N_HIST_IMAGES, CHANNELS // 2 of temporal_conv
TIME_PARAM_SHAPES = ((TIME_C, 1, 1, 2), (TIME_C,), (TIME_C, TIME_C, 1, 2), (TIME_C,), (1, TIME_C, 1, 2), (1,))


def _check_frame_stripe(who, history, stripe_start, weight_shape, stripe_width):
    """The shape rule of pv_conv2d_ae_frame_stripe_*: history [N, F, H, W] (F = 1..7), stripe_start int32 [N], weight [16, 2,
    3, 3].  Returns the entry points' (n, frames, h, w) and the output's shape."""
    n, frames, h, w = _check_stripe(who, history, stripe_start, stripe_width)
    if tuple(weight_shape) != (FRAME_STRIPE_C_OUT, 2, 3, 3):
        raise ValueError(f"{who}: weight [{FRAME_STRIPE_C_OUT}, 2, 3, 3] expected, got {tuple(weight_shape)}")
    return (int(n), int(frames), int(h), int(w)), (n * frames, FRAME_STRIPE_C_OUT, *_CONV2D_AE.out_hw(h, w))


def conv2d_ae_frame_stripe_fwd_f32(history, stripe_start, weight, bias, stripe_width):
    """relu(conv2d(cat(history[:, f:f + 1], stripe plane), weight) + bias) for every frame f at once: history [N, F, H, W] f32
    read in place, the stripe plane of example i is 1 on columns stripe_start[i] <= c < stripe_start[i] + stripe_width (inside
    the image) -> [N F, 16, H - 2, W - 2] with image index F i + f; weight [16, 2, 3, 3]."""
    who = "conv2d_ae_frame_stripe_fwd_f32"
    dims, y_shape = _check_frame_stripe(who, history, stripe_start, weight.shape, stripe_width)
    if bias is None or tuple(bias.shape) != (FRAME_STRIPE_C_OUT,):
        raise ValueError(f"{who}: bias [{FRAME_STRIPE_C_OUT}] expected")
    require_cuda(weight, bias)
    _f32_contig(weight, bias)
    y = torch.empty(y_shape, dtype=torch.float32, device=history.device)
    check(get_lib().pv_conv2d_ae_frame_stripe_fwd_f32(ptr(history), ptr(stripe_start), ptr(weight), ptr(bias), ptr(y), *dims,
                                                      FRAME_STRIPE_C_OUT, int(stripe_width), current_stream_ptr()),
          "pv_" + who)
    return y


def conv2d_ae_frame_stripe_bwd_weight_f32(history, stripe_start, dy, weight_shape, stripe_width):
    """(dw [16, 2, 3, 3], dbias [16]) of conv2d_ae_frame_stripe_fwd_f32's conv, summed over its frames, from its pre-activation
    gradient dy [N F, 16, H - 2, W - 2]; deterministic."""
    who = "conv2d_ae_frame_stripe_bwd_weight_f32"
    dims, y_shape = _check_frame_stripe(who, history, stripe_start, weight_shape, stripe_width)
    if tuple(dy.shape) != y_shape:
        raise ValueError(f"{who}: dy {y_shape} expected, got {tuple(dy.shape)}")
    require_cuda(dy)
    _f32_contig(dy)
    ws, nbytes = _wgrad_ws("conv2d_ae_frame_stripe", history.device, *dims)
    dw, db = _grads_out(weight_shape, FRAME_STRIPE_C_OUT, history.device)
    check(get_lib().pv_conv2d_ae_frame_stripe_bwd_weight_f32(ptr(history), ptr(stripe_start), ptr(dy), ptr(dw), ptr(db), *dims,
                                                             FRAME_STRIPE_C_OUT, int(stripe_width), ptr(ws), nbytes,
                                                             current_stream_ptr()), "pv_" + who)
    return dw, db


def _check_conv_time(who, u, params):
    """The shape rule of pv_conv_time_*: u [4 N, 1, H, W] (the per-frame stack's output, image 4 i + f) and temporal_conv's six
    parameters.  Returns the entry points' (n, frames, c_mid, p)."""
    if u.dim() != 4 or u.shape[1] != 1 or u.shape[0] % TIME_FRAMES or u.numel() == 0:
        raise ValueError(f"{who}: u [{TIME_FRAMES} N, 1, H, W] expected, got {tuple(u.shape)}")
    got = tuple(tuple(t.shape) for t in params)
    if got != TIME_PARAM_SHAPES[:len(got)]:
        raise ValueError(f"{who}: parameters {TIME_PARAM_SHAPES[:len(got)]} expected, got {got}")
    require_cuda(u, *params)
    _f32_contig(u, *params)
    return u.shape[0] // TIME_FRAMES, TIME_FRAMES, TIME_C, u.shape[2] * u.shape[3]


def conv_time_fwd_f32(u, w1, b1, w2, b2, w3, b3):
    """temporal_conv of notebook 11 per pixel: u [4 N, 1, H, W] f32 holds the four frames' values of example i in images 4 i ..
    4 i + 3; conv2d (1, 2) 1 -> 16, ReLU, 16 -> 16, ReLU, 16 -> 1 over the frame axis -> [N, 1, H, W]."""
    who = "conv_time_fwd_f32"
    dims = _check_conv_time(who, u, (w1, b1, w2, b2, w3, b3))
    y = torch.empty((dims[0], 1, *u.shape[2:]), dtype=torch.float32, device=u.device)
    check(get_lib().pv_conv_time_fwd_f32(ptr(u), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(w3), ptr(b3), ptr(y), *dims,
                                         current_stream_ptr()), "pv_" + who)
    return y


def conv_time_bwd_f32(u, dy, w1, b1, w2, b2, w3, u_is_relu_output=False):
    """(du [4 N, 1, H, W], dw1, db1, dw2, db2, dw3, db3) of conv_time_fwd_f32 from dy [N, 1, H, W]: the hidden layers are
    recomputed from u and gated by the recomputed values; deterministic (per-block partial sums added in order).
    u_is_relu_output: du leaves zeroed where u <= 0 (the pre-activation gradient of the ReLU that made u)."""
    who = "conv_time_bwd_f32"
    dims = _check_conv_time(who, u, (w1, b1, w2, b2, w3))
    y_shape = (dims[0], 1, *u.shape[2:])
    if tuple(dy.shape) != y_shape:
        raise ValueError(f"{who}: dy {y_shape} expected, got {tuple(dy.shape)}")
    require_cuda(dy)
    _f32_contig(dy)
    query = "pv_conv_time_bwd_workspace_bytes"
    nbytes = ctypes.c_size_t(0)
    check(getattr(get_lib(), query)(*dims, ctypes.byref(nbytes)), query)
    ws = _workspace("conv_time_bwd", nbytes.value, u.device)
    du = torch.empty_like(u)
    grads = tuple(torch.empty(shape, dtype=torch.float32, device=u.device) for shape in TIME_PARAM_SHAPES)
    check(get_lib().pv_conv_time_bwd_f32(ptr(u), ptr(dy), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(w3), ptr(du),
                                         *(ptr(g) for g in grads), *dims, int(bool(u_is_relu_output)), ptr(ws), nbytes.value,
                                         current_stream_ptr()),
          "pv_" + who)
    return (du, *grads)


def maxpool3d_fwd_f32(x, kernel=3, stride=None, padding=0):
    require_cuda(x)
    b, c, t, h, w = x.shape
    g = conv_geom(b, c, c, t, h, w, kernel, kernel if stride is None else stride, padding)
    y = torch.empty((b, c) + g.out_shape(), dtype=torch.float32, device=x.device)
    idx = torch.empty(y.shape, dtype=torch.int32, device=x.device)
    check(get_lib().pv_maxpool3d_fwd_f32(ptr(x), ptr(y), ptr(idx), ctypes.byref(g), current_stream_ptr()),
          "pv_maxpool3d_fwd_f32")
    return y, idx, g


def maxpool3d_bwd_f32(dy, idx, g: Conv3dGeom):
    require_cuda(dy, idx)
    dx = torch.empty((g.batch, g.c_in, g.t_in, g.h_in, g.w_in), dtype=torch.float32, device=dy.device)
    check(get_lib().pv_maxpool3d_bwd_f32(ptr(dy), ptr(idx), ptr(dx), ctypes.byref(g), current_stream_ptr()),
          "pv_maxpool3d_bwd_f32")
    return dx


def mse_loss(y_hat, y, need_grad=True, grad_scale=1.0):
    require_cuda(y_hat, y)
    if y_hat.shape != y.shape:
        raise ValueError(f"mse_loss: shapes differ: {tuple(y_hat.shape)} vs {tuple(y.shape)}")
    out = torch.empty((1,), dtype=torch.float32, device=y_hat.device)
    grad = torch.empty_like(y_hat) if need_grad else None
    check(get_lib().pv_mse_loss_f32(ptr(y_hat), ptr(y), y_hat.numel(), float(grad_scale), ptr(out), ptr(grad),
                                    current_stream_ptr()), "pv_mse_loss_f32")
    return out, grad


# ---- Perceiver path: strided batched GEMM on the f32 matrix cores + row-wise kernels -----------------------------------
def _require_device(*tensors):
    """Like require_cuda but for STRIDED views: the GEMM reads its operands through explicit element strides."""
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("predict_pv_yield_amd: tensors must live on the MI355X (no CPU path is provided)")


def _gemm_views(a: torch.Tensor, b: torch.Tensor):
    """a [..., M, K], b [..., K, N] with the same (<= 2) leading batch dims (stride-0 broadcast allowed)."""
    if a.dim() != b.dim() or a.dim() < 2 or a.dim() > 4 or a.shape[:-2] != b.shape[:-2] or a.shape[-1] != b.shape[-2]:
        raise ValueError(f"gemm: incompatible shapes {tuple(a.shape)} x {tuple(b.shape)}")
    if a.dtype not in (torch.float32, torch.bfloat16) or b.dtype != torch.float32:      # (a bf16 A: see gemm's bf16_operands)
        raise TypeError("gemm: float32 operands expected")
    batch = tuple(a.shape[:-2])
    while len(batch) < 2:
        a, b, batch = a.unsqueeze(0), b.unsqueeze(0), (1,) + batch
    return a, b, batch


GEMM_BF16_OPERANDS = 1      # PV_GEMM_BF16_OPERANDS of include/pv_yield_hip.h
GEMM_A_IS_BF16 = 2          # PV_GEMM_A_IS_BF16


def gemm(a: torch.Tensor, b: torch.Tensor, bias: Optional[torch.Tensor] = None, relu: bool = False,
         out: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None, bf16_operands: bool = False) -> torch.Tensor:
    """C = A @ B (+ bias) (+ residual) for arbitrarily STRIDED views (transposes, column slices and per-head permutes are
    free: only the strides change).  `out`: optional view [..., M, N] with unit last stride to write into.
    `residual`: a [M, N] tensor with unit last stride added in the epilogue (2-D products only).
    bf16_operands: both operands rounded once to bf16, one matrix-core product, f32 accumulation (torch.autocast's linear);
    default: the f32-accurate three-term form."""
    _require_device(a, b, out, residual)
    require_cuda(bias)
    a_bf16 = a.dtype == torch.bfloat16      # (with bf16_operands: A may be STORED as bf16 -- read as it is)
    if a_bf16 and not bf16_operands:
        raise ValueError("gemm: a bfloat16 A needs bf16_operands=True")
    lead = tuple(a.shape[:-2])
    a4, b4, batch = _gemm_views(a, b)
    m, k, n = a4.shape[-2], a4.shape[-1], b4.shape[-1]
    if out is None:
        out = torch.empty(lead + (m, n), dtype=torch.float32, device=a.device)
    c4 = out
    while c4.dim() < 4:
        c4 = c4.unsqueeze(0)
    if tuple(c4.shape) != batch + (m, n) or c4.stride(-1) != 1:
        raise ValueError("gemm: bad output view")
    d = _lib.GemmDesc(m, n, k, a4.stride(-2), a4.stride(-1), b4.stride(-2), b4.stride(-1), c4.stride(-2), batch[0], batch[1],
                      a4.stride(0), a4.stride(1), b4.stride(0), b4.stride(1), c4.stride(0), c4.stride(1), 1, 0)
    if residual is not None:
        if batch != (1, 1) or tuple(residual.shape) != (m, n) or residual.stride(-1) != 1 or residual.dtype != torch.float32:
            raise ValueError("gemm: residual must be a float32 [M, N] tensor with unit last stride (2-D products only)")
    check(get_lib().pv_gemm_ex_f32(ptr(a4), ptr(b4), ptr(bias), ptr(residual), residual.stride(0) if residual is not None else 0,
                                   ptr(c4), ctypes.byref(d), int(relu),
                                   (GEMM_BF16_OPERANDS if bf16_operands else 0) | (GEMM_A_IS_BF16 if a_bf16 else 0),
                                   current_stream_ptr()), "pv_gemm_ex_f32")
    return out


def gemm_rows_bf16out_supported(a: torch.Tensor, b: torch.Tensor) -> bool:
    """pv_gemm_rows_bf16out_f32's shape rule: one tall row-major A [M, K <= 64] (16-byte aligned), B [K, N]."""
    return (a.dim() == 2 and b.dim() == 2 and a.dtype == torch.float32 and a.stride(1) == 1 and a.shape[1] <= 64
            and a.shape[0] >= 2048 and a.data_ptr() % 16 == 0)


def gemm_rows_bf16out(a: torch.Tensor, b: torch.Tensor, bias: Optional[torch.Tensor] = None, bf16_operands: bool = False) -> torch.Tensor:
    """C (bf16) = A @ B (+ bias) for a tall row-major A with K <= 64: f32-accurate products, ONE rounding in the store (the
    key / value projection of a cross-attention in bf16-operand mode)."""
    _require_device(a, b)
    require_cuda(bias)
    if not gemm_rows_bf16out_supported(a, b):
        raise ValueError("gemm_rows_bf16out: a tall row-major float32 A [M >= 2048, K <= 64] is expected")
    m, k, n = a.shape[0], a.shape[1], b.shape[1]
    out = torch.empty((m, n), dtype=torch.bfloat16, device=a.device)
    d = _lib.GemmDesc(m, n, k, a.stride(0), a.stride(1), b.stride(0), b.stride(1), n, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0)
    check(get_lib().pv_gemm_rows_bf16out_f32(ptr(a), ptr(b), ptr(bias), ptr(out), ctypes.byref(d),
                                             GEMM_BF16_OPERANDS if bf16_operands else 0, current_stream_ptr()),
          "pv_gemm_rows_bf16out_f32")
    return out


# split-K sizing: enough workgroups to fill the chip, but a K chunk long enough to amortise a workgroup's fixed costs
SPLITK_TARGET_WORKGROUPS = 1024
SPLITK_MIN_CHUNK = 256


def gemm_splitk(a: torch.Tensor, b: torch.Tensor, accumulate_into: Optional[torch.Tensor] = None,
                bf16_operands: bool = False) -> torch.Tensor:
    """C[M, N] = A[M, K] @ B[K, N] for small M, N and a huge K (weight gradients): K is cut over workgroups, the partial
    products are summed in index order (deterministic).  accumulate_into: a contiguous [M, N] tensor that receives
    `+= C` (the slab sum adds into it) and is returned."""
    _require_device(a, b, accumulate_into)
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[0]:
        raise ValueError(f"gemm_splitk: incompatible shapes {tuple(a.shape)} x {tuple(b.shape)}")
    m, k, n = a.shape[0], a.shape[1], b.shape[1]
    if accumulate_into is not None and (tuple(accumulate_into.shape) != (m, n) or not accumulate_into.is_contiguous()):
        raise ValueError("gemm_splitk: accumulate_into must be a contiguous [M, N] tensor")
    tiles = ((m + 127) // 128) * ((n + 63) // 64)
    splits = max(1, min((SPLITK_TARGET_WORKGROUPS + tiles - 1) // tiles, (k + SPLITK_MIN_CHUNK - 1) // SPLITK_MIN_CHUNK, 4096))
    if splits == 1 and accumulate_into is None:
        return gemm(a, b, bf16_operands=bf16_operands)
    slabs = _workspace("gemm_splitk", splits * m * n * 4, a.device)
    d = _lib.GemmDesc(m, n, k, a.stride(0), a.stride(1), b.stride(0), b.stride(1), n, 1, 1, 0, 0, 0, 0, 0, 0, splits, m * n)
    a_bf16 = a.dtype == torch.bfloat16
    if a_bf16 and not bf16_operands:
        raise ValueError("gemm_splitk: a bfloat16 A needs bf16_operands=True")
    check(get_lib().pv_gemm_ex_f32(ptr(a), ptr(b), None, None, 0, ptr(slabs), ctypes.byref(d), 0,
                                   (GEMM_BF16_OPERANDS if bf16_operands else 0) | (GEMM_A_IS_BF16 if a_bf16 else 0),
                                   current_stream_ptr()), "pv_gemm_ex_f32")
    out = accumulate_into if accumulate_into is not None else torch.empty((m, n), dtype=torch.float32, device=a.device)
    check(get_lib().pv_sum_slabs_acc_f32(ptr(slabs), ptr(out), m * n, splits, int(accumulate_into is not None),
                                         current_stream_ptr()), "pv_sum_slabs_acc_f32")
    return out


def colsum(x: torch.Tensor, accumulate_into: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Column sums of a contiguous [rows, cols] tensor (the bias gradient of nn.Linear), chunk partials added in order."""
    require_cuda(x, accumulate_into)
    if x.dim() != 2 or x.dtype != torch.float32:
        raise TypeError("colsum: a contiguous float32 [rows, cols] tensor is expected")
    rows, cols = x.shape
    n_ws = get_lib().pv_colsum_workspace_floats(rows, cols)
    ws = _workspace("colsum", n_ws * 4, x.device)
    out = accumulate_into if accumulate_into is not None else torch.empty(cols, dtype=torch.float32, device=x.device)
    check(get_lib().pv_colsum_f32(ptr(x), ptr(out), rows, cols, ptr(ws), int(accumulate_into is not None),
                                  current_stream_ptr()), "pv_colsum_f32")
    return out


def layernorm_fwd(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float = 1e-5):
    require_cuda(x, w, b)
    d = x.shape[-1]
    rows = x.numel() // d
    y = torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    check(get_lib().pv_layernorm_fwd_f32(ptr(x), ptr(w), ptr(b), ptr(y), ptr(mean), ptr(rstd), rows, d, eps,
                                         current_stream_ptr()), "pv_layernorm_fwd_f32")
    return y, mean, rstd


def layernorm_bwd(x, w, dy, mean, rstd, need_dx: bool = True, accumulate_into=None, dx_add=None):
    """-> (dx | None, dw, db).  For d % 4 == 0, dw and db are the two halves of ONE [2 d] tensor (one reduction launch).
    accumulate_into: a (dw, db) pair returned by an earlier call, which receives `+=` instead.
    dx_add: a tensor like x added to dx in the kernel's store (the gradient that reaches x past the normalised branch)."""
    require_cuda(x, w, dy, mean, rstd, dx_add)
    if dx_add is not None and (not need_dx or dx_add.shape != x.shape or not dx_add.is_contiguous()):
        raise ValueError("layernorm_bwd: dx_add must be a contiguous tensor like x (and need_dx)")
    d = x.shape[-1]
    rows = x.numel() // d
    nbytes = ctypes.c_size_t(0)
    check(get_lib().pv_layernorm_bwd_workspace_bytes(rows, d, ctypes.byref(nbytes)), "pv_layernorm_bwd_workspace_bytes")
    ws = _workspace("layernorm_bwd", nbytes.value, x.device)
    dx = torch.empty_like(x) if need_dx else None
    if accumulate_into is not None:
        dw, db = accumulate_into
    elif d % 4 == 0:     # halves of one buffer stay 16-byte aligned (the optimizer kernels require it)
        dwdb = torch.empty(2 * d, dtype=torch.float32, device=x.device)
        dw, db = dwdb[:d], dwdb[d:]
    else:
        dw = torch.empty(d, dtype=torch.float32, device=x.device)
        db = torch.empty(d, dtype=torch.float32, device=x.device)
    check(get_lib().pv_layernorm_bwd_f32(ptr(x), ptr(w), ptr(dy), ptr(mean), ptr(rstd), ptr(dx), ptr(dw), ptr(db), rows, d,
                                         ptr(ws), nbytes.value, int(accumulate_into is not None), ptr(dx_add),
                                         current_stream_ptr()), "pv_layernorm_bwd_f32")
    return dx, dw, db


def layernorm_bwd_params_from_proj_supported(dkv16: torch.Tensor, w_kv: torch.Tensor, x: torch.Tensor) -> bool:
    return (dkv16.dtype == torch.bfloat16 and dkv16.is_contiguous() and w_kv.is_contiguous() and x.is_contiguous()
            and x.dtype == torch.float32 and w_kv.dtype == torch.float32 and w_kv.shape[0] in (64, 128)
            and x.shape[-1] == w_kv.shape[1] <= 64 and dkv16.shape[-1] == w_kv.shape[0]
            and dkv16.numel() // dkv16.shape[-1] == x.numel() // x.shape[-1] and dkv16.data_ptr() % 16 == 0)


def layernorm_bwd_params_from_proj(dkv16, w_kv, x, mean, rstd, accumulate_into=None):
    """(dw, db) of the LayerNorm in  x -> LayerNorm -> to_kv  from the bf16 gradient of the projection, d(LayerNorm output)
    never materialised (pv_layernorm_bwd_params_from_proj_bf16).  dw / db as layernorm_bwd returns them."""
    require_cuda(dkv16, w_kv, x, mean, rstd)
    if not layernorm_bwd_params_from_proj_supported(dkv16, w_kv, x):
        raise ValueError("layernorm_bwd_params_from_proj: bf16 gradient rows [rows, 64 | 128], f32 weight [kdim, d <= 64], f32 x")
    d = x.shape[-1]
    rows = x.numel() // d
    nbytes = ctypes.c_size_t(0)
    check(get_lib().pv_layernorm_bwd_params_from_proj_workspace_bytes(rows, d, ctypes.byref(nbytes)),
          "pv_layernorm_bwd_params_from_proj_workspace_bytes")
    ws = _workspace("layernorm_bwd_proj", nbytes.value, x.device)
    if accumulate_into is not None:
        dw, db = accumulate_into
    elif d % 4 == 0:
        dwdb = torch.empty(2 * d, dtype=torch.float32, device=x.device)
        dw, db = dwdb[:d], dwdb[d:]
    else:
        dw = torch.empty(d, dtype=torch.float32, device=x.device)
        db = torch.empty(d, dtype=torch.float32, device=x.device)
    check(get_lib().pv_layernorm_bwd_params_from_proj_bf16(ptr(dkv16), ptr(w_kv), ptr(x), ptr(mean), ptr(rstd), ptr(dw), ptr(db),
                                                           rows, d, w_kv.shape[0], ptr(ws), nbytes.value,
                                                           int(accumulate_into is not None), current_stream_ptr()),
          "pv_layernorm_bwd_params_from_proj_bf16")
    return dw, db


def _context_rows(x: torch.Tensor, x2):
    """(rows, d, d1, period) of a context given as x [..., d] or as x [..., P, d1] + x2 [P, d2] (row r = x row r followed by
    x2 row r % P: image channels + the position features every image shares)."""
    d1 = x.shape[-1]
    rows = x.numel() // d1
    if x2 is None:
        return rows, d1, 0, 0
    return rows, d1 + x2.shape[-1], d1, x2.shape[0]


def context_fwd_supported(x: torch.Tensor, w_kv: torch.Tensor, x2=None) -> bool:
    rows, d, d1, period = _context_rows(x, x2)
    # (period >= 32: pv_context_bwd_bf16's rule -- a forward the backward cannot follow must not be chosen)
    if x2 is not None and not (x2.dim() == 2 and x2.dtype == torch.float32 and x2.is_contiguous() and x.dim() >= 2
                               and x.shape[-2] == period and period >= 32 and d1 % 2 == 0 and x2.data_ptr() % 8 == 0
                               and x2.device == x.device):
        return False
    return (x.dtype == torch.float32 and x.is_contiguous() and w_kv.is_contiguous() and w_kv.dtype == torch.float32
            and w_kv.shape[0] == 128 and d == w_kv.shape[1] <= 48 and d % 2 == 0
            and x.data_ptr() % 16 == 0 and 2048 <= rows < 2 ** 31)


def context_fwd(x, ln_w, ln_b, w_kv, eps: float = 1e-5, x2=None):
    """K | V (bf16) = LayerNorm(context) @ w_kv^T in one pass (pv_context_fwd_bf16) -> (kv16 [..., 128], mean, rstd).
    context = x [..., d], or x [..., P, d1] with x2 [P, d2] appended to every group of P rows (never concatenated in memory)."""
    require_cuda(x, ln_w, ln_b, w_kv, x2)
    if not context_fwd_supported(x, w_kv, x2):
        raise ValueError("context_fwd: contiguous f32 x [..., d <= 48, even] (or x [..., P, d1] + x2 [P, d2]) and w_kv [128, d] expected")
    rows, d, d1, period = _context_rows(x, x2)
    kv16 = torch.empty(x.shape[:-1] + (128,), dtype=torch.bfloat16, device=x.device)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    check(get_lib().pv_context_fwd_bf16(ptr(x), ptr(x2), d1, period, ptr(ln_w), ptr(ln_b), ptr(w_kv), ptr(kv16), ptr(mean),
                                        ptr(rstd), rows, d, 128, float(eps), current_stream_ptr()), "pv_context_fwd_bf16")
    return kv16, mean, rstd


def context_bwd_supported(dkv16: torch.Tensor, w_kv: torch.Tensor, x: torch.Tensor, x2=None) -> bool:
    rows, d, d1, period = _context_rows(x, x2)
    if x2 is not None and not (x2.dim() == 2 and x2.dtype == torch.float32 and x2.is_contiguous() and x.dim() >= 2
                               and x.shape[-2] == period and period >= 32 and x2.device == x.device):
        return False
    return (dkv16.dtype == torch.bfloat16 and dkv16.is_contiguous() and w_kv.is_contiguous() and x.is_contiguous()
            and x.dtype == torch.float32 and w_kv.dtype == torch.float32 and w_kv.shape[0] == 128 and d == w_kv.shape[1] <= 64
            and dkv16.shape[-1] == 128 and dkv16.numel() // 128 == rows < 2 ** 31 and dkv16.data_ptr() % 16 == 0)


def context_bwd(dkv16, w_kv, x, mean, rstd, ln_w, ln_b, accumulate_kv_into=None, accumulate_ln_into=None, x2=None):
    """The backward of  context -> LayerNorm -> to_kv  for a context that takes no gradient, from the bf16 gradient rows of K | V,
    in one pass (pv_context_bwd_bf16): -> (dw_kv [128, d], dln_w, dln_b).  accumulate_*_into: tensors that receive `+=` instead.
    x2: as in context_fwd."""
    require_cuda(dkv16, w_kv, x, mean, rstd, ln_w, ln_b, x2)
    if not context_bwd_supported(dkv16, w_kv, x, x2):
        raise ValueError("context_bwd: bf16 gradient rows [rows, 128], f32 weight [128, d <= 64], f32 context rows")
    rows, d, d1, period = _context_rows(x, x2)
    nbytes = ctypes.c_size_t(0)
    check(get_lib().pv_context_bwd_workspace_bytes(rows, d, ctypes.byref(nbytes)), "pv_context_bwd_workspace_bytes")
    ws = _workspace("context_bwd", nbytes.value, x.device)
    dw = accumulate_kv_into if accumulate_kv_into is not None else torch.empty_like(w_kv)
    if accumulate_ln_into is not None:
        dlw, dlb = accumulate_ln_into
    elif d % 4 == 0:
        both = torch.empty(2 * d, dtype=torch.float32, device=x.device)
        dlw, dlb = both[:d], both[d:]
    else:
        dlw = torch.empty(d, dtype=torch.float32, device=x.device)
        dlb = torch.empty(d, dtype=torch.float32, device=x.device)
    check(get_lib().pv_context_bwd_bf16(ptr(dkv16), ptr(w_kv), ptr(x), ptr(x2), d1, period, ptr(mean), ptr(rstd), ptr(ln_w),
                                        ptr(ln_b), ptr(dw), ptr(dlw), ptr(dlb), rows, d, w_kv.shape[0], ptr(ws), nbytes.value,
                                        int(accumulate_kv_into is not None), int(accumulate_ln_into is not None),
                                        current_stream_ptr()), "pv_context_bwd_bf16")
    return dw, dlw, dlb


def softmax_fwd_(x: torch.Tensor, scale: float) -> torch.Tensor:
    """In place: x <- softmax(scale * x) over the last dimension (contiguous)."""
    require_cuda(x)
    n = x.shape[-1]
    check(get_lib().pv_softmax_fwd_f32(ptr(x), ptr(x), x.numel() // n, n, scale, current_stream_ptr()), "pv_softmax_fwd_f32")
    return x


def softmax_bwd_(p: torch.Tensor, dp: torch.Tensor, scale: float) -> torch.Tensor:
    """In place on dp: dp <- scale * p * (dp - sum(dp * p))."""
    require_cuda(p, dp)
    n = p.shape[-1]
    check(get_lib().pv_softmax_bwd_f32(ptr(p), ptr(dp), ptr(dp), p.numel() // n, n, scale, current_stream_ptr()),
          "pv_softmax_bwd_f32")
    return dp


def geglu_fwd(x: torch.Tensor) -> torch.Tensor:
    require_cuda(x)
    h = x.shape[-1] // 2
    y = torch.empty(x.shape[:-1] + (h,), dtype=torch.float32, device=x.device)
    check(get_lib().pv_geglu_fwd_f32(ptr(x), ptr(y), x.numel() // (2 * h), h, current_stream_ptr()), "pv_geglu_fwd_f32")
    return y


def geglu_bwd(x: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    require_cuda(x, dy)
    h = x.shape[-1] // 2
    dx = torch.empty_like(x)
    check(get_lib().pv_geglu_bwd_f32(ptr(x), ptr(dy), ptr(dx), x.numel() // (2 * h), h, current_stream_ptr()), "pv_geglu_bwd_f32")
    return dx


def mean_axis1_fwd(x: torch.Tensor) -> torch.Tensor:
    require_cuda(x)
    b, n, d = x.shape
    y = torch.empty((b, d), dtype=torch.float32, device=x.device)
    check(get_lib().pv_mean_axis1_fwd_f32(ptr(x), ptr(y), b, n, d, current_stream_ptr()), "pv_mean_axis1_fwd_f32")
    return y


def mean_axis1_bwd(dy: torch.Tensor, n: int) -> torch.Tensor:
    require_cuda(dy)
    b, d = dy.shape
    dx = torch.empty((b, n, d), dtype=torch.float32, device=dy.device)
    check(get_lib().pv_mean_axis1_bwd_f32(ptr(dy), ptr(dx), b, n, d, current_stream_ptr()), "pv_mean_axis1_bwd_f32")
    return dx


def gru_seq_fwd(gi: torch.Tensor, h0: Optional[torch.Tensor], w_hh: torch.Tensor, b_hh: torch.Tensor):
    require_cuda(gi, h0, w_hh, b_hh)
    b, t, h3 = gi.shape
    h = h3 // 3
    out = torch.empty((b, t, h), dtype=torch.float32, device=gi.device)
    saved = torch.empty((b, t, 4 * h), dtype=torch.float32, device=gi.device)
    check(get_lib().pv_gru_seq_fwd_f32(ptr(gi), ptr(h0), ptr(w_hh), ptr(b_hh), ptr(out), ptr(saved), b, t, h,
                                       current_stream_ptr()), "pv_gru_seq_fwd_f32")
    return out, saved


def gru_seq_bwd(dout, dh_last, h0, out, saved, w_hh, need_dh0: bool):
    require_cuda(dout, dh_last, h0, out, saved, w_hh)
    b, t, h = out.shape
    dgi = torch.empty((b, t, 3 * h), dtype=torch.float32, device=out.device)
    dh0 = torch.empty((b, h), dtype=torch.float32, device=out.device) if need_dh0 else None
    dw = torch.empty((3 * h, h), dtype=torch.float32, device=out.device)
    db = torch.empty((3 * h,), dtype=torch.float32, device=out.device)
    nbytes = b * (3 * h * h + 3 * h) * 4
    ws = _workspace("gru_bwd", nbytes, out.device)
    check(get_lib().pv_gru_seq_bwd_f32(ptr(dout), ptr(dh_last), ptr(h0), ptr(out), ptr(saved), ptr(w_hh), ptr(dgi), ptr(dh0),
                                       ptr(dw), ptr(db), b, t, h, ptr(ws), nbytes, current_stream_ptr()), "pv_gru_seq_bwd_f32")
    return dgi, dh0, dw, db


def attention_desc(q: torch.Tensor, kv: torch.Tensor, heads: int, scale: float) -> "_lib.AttentionDesc":
    b, n_q, inner = q.shape
    return _lib.AttentionDesc(b, heads, n_q, kv.shape[1], inner // heads, q.stride(0), q.stride(1), kv.stride(0), kv.stride(1),
                              scale)


def attention_fwd(q: torch.Tensor, kv: torch.Tensor, heads: int, scale: float, bf16_operands: bool = False):
    """q [b, i, h*64], kv [b, j, 2*h*64] (k | v halves) contiguous -> (out [b, i, h*64], lse [b, h, i]).
    bf16_operands: the two products take bf16 operands on the bf16 matrix cores (f32 accumulation, f32 softmax)."""
    require_cuda(q, kv)
    b, n_q, inner = q.shape
    d = attention_desc(q, kv, heads, scale)
    out = torch.empty_like(q)
    lse = torch.empty((b, heads, n_q), dtype=torch.float32, device=q.device)
    kv16 = kv.dtype == torch.bfloat16      # K / V stored as bf16 (gemm_rows_bf16out): bf16-operand kernels only
    if kv16 and not bf16_operands:
        raise ValueError("attention_fwd: a bfloat16 kv needs bf16_operands=True")
    v_ptr = ctypes.c_void_p(kv.data_ptr() + inner * kv.element_size())
    if bf16_operands:
        n_ws = get_lib().pv_attention_fwd_workspace_floats(ctypes.byref(d))
        ws = _workspace("attention_fwd", n_ws * 4, q.device) if n_ws else None
        fn = get_lib().pv_attention_fwd_bf16kv if kv16 else get_lib().pv_attention_fwd_bf16
        check(fn(ptr(q), ptr(kv), v_ptr, ptr(out), ptr(lse), ctypes.byref(d), ptr(ws), current_stream_ptr()),
              "pv_attention_fwd_bf16kv" if kv16 else "pv_attention_fwd_bf16")
    else:
        check(get_lib().pv_attention_fwd_f32(ptr(q), ptr(kv), v_ptr, ptr(out), ptr(lse), ctypes.byref(d), current_stream_ptr()),
              "pv_attention_fwd_f32")
    return out, lse


def attention_bwd(q, kv, out, dout, lse, heads: int, scale: float, bf16_operands: bool = False, accumulate_dkv_into=None,
                  dkv_bf16: bool = False):
    """Backward of attention_fwd (n_q <= 128): returns (dq like q, dkv like kv).
    accumulate_dkv_into (bf16 operands only): a tensor like kv that receives `+= dkv` in the kernel's store.
    dkv_bf16 (bf16-stored kv only): dkv is STORED as bf16 too -- for a consumer that rounds it to bf16 anyway."""
    require_cuda(q, kv, out, dout, lse, accumulate_dkv_into)
    b, n_q, inner = q.shape
    d = attention_desc(q, kv, heads, scale)
    dq = torch.empty_like(q)
    kv16 = kv.dtype == torch.bfloat16
    if kv16 and not bf16_operands:
        raise ValueError("attention_bwd: a bfloat16 kv needs bf16_operands=True")
    if dkv_bf16:
        if not kv16 or accumulate_dkv_into is not None:
            raise ValueError("attention_bwd: dkv_bf16 needs a bfloat16 kv and no accumulate_dkv_into")
        dkv = torch.empty(kv.shape, dtype=torch.bfloat16, device=kv.device)
        n_ws = get_lib().pv_attention_bwd_workspace_floats(ctypes.byref(d))
        delta = _workspace("attention_bwd", n_ws * 4, q.device)
        check(get_lib().pv_attention_bwd_bf16kv16(ptr(q), ptr(kv), ctypes.c_void_p(kv.data_ptr() + inner * 2), ptr(out), ptr(dout),
                                                  ptr(lse), ptr(delta), ptr(dq), ptr(dkv),
                                                  ctypes.c_void_p(dkv.data_ptr() + inner * 2), ctypes.byref(d),
                                                  current_stream_ptr()), "pv_attention_bwd_bf16kv16")
        return dq, dkv
    if accumulate_dkv_into is not None:
        if (not bf16_operands or accumulate_dkv_into.shape != kv.shape or not accumulate_dkv_into.is_contiguous()
                or accumulate_dkv_into.dtype != torch.float32):
            raise ValueError("attention_bwd: accumulate_dkv_into needs the bf16-operand kernels and a contiguous float32 tensor "
                             "shaped like kv")
        dkv = accumulate_dkv_into
    else:
        dkv = torch.empty(kv.shape, dtype=torch.float32, device=kv.device)
    n_ws = get_lib().pv_attention_bwd_workspace_floats(ctypes.byref(d))
    delta = _workspace("attention_bwd", n_ws * 4, q.device)
    v_ptr = ctypes.c_void_p(kv.data_ptr() + inner * kv.element_size())
    dv_ptr = ctypes.c_void_p(dkv.data_ptr() + inner * 4)
    if bf16_operands:
        fn = get_lib().pv_attention_bwd_bf16kv if kv16 else get_lib().pv_attention_bwd_bf16
        check(fn(ptr(q), ptr(kv), v_ptr, ptr(out), ptr(dout), ptr(lse), ptr(delta), ptr(dq), ptr(dkv), dv_ptr, ctypes.byref(d),
                 int(accumulate_dkv_into is not None), current_stream_ptr()),
              "pv_attention_bwd_bf16kv" if kv16 else "pv_attention_bwd_bf16")
    else:
        check(get_lib().pv_attention_bwd_f32(ptr(q), ptr(kv), v_ptr, ptr(out), ptr(dout), ptr(lse), ptr(delta), ptr(dq), ptr(dkv),
                                             dv_ptr, ctypes.byref(d), current_stream_ptr()), "pv_attention_bwd_f32")
    return dq, dkv
