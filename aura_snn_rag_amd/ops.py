"""Tensor-level wrappers over the C ABI (``include/aura_hip.h``).

Every function takes HIP-resident, contiguous torch tensors, checks shapes/dtypes on the host
(a bad shape reaching a hand-written kernel can fault the GPU) and launches on torch's current
stream.  There is no fallback: CPU tensors raise ``AuraDeviceError``.
"""
from __future__ import annotations

import ctypes
import time
import warnings
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check, KNN_FLAG_LISTS_STALE, KNN_FLAG_NO_CANDIDATES


class AuraDeviceError(RuntimeError):
    """Raised when a hot-path op is asked to run on something that is not a HIP device."""


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _need(t: torch.Tensor, name: str, dtype=None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(t)}")
    if not t.is_cuda:
        raise AuraDeviceError(
            f"{name} is on {t.device}: aura_snn_rag_amd runs the hot path only as HIP kernels on "
            f"an AMD GPU (no CPU/PyTorch fallback).")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t


def _need_image(t: torch.Tensor, name: str) -> int:
    """A 16-bit image of normalised rows: bf16, or IEEE half (the list-sorted image of the inverted lists).  Returns
    the C ABI's ``image_format`` of its dtype, ``_lib.IMAGE_BF16`` or ``_lib.IMAGE_F16``."""
    _need(t, name)
    if t.dtype not in (torch.bfloat16, torch.float16):
        raise TypeError(f"{name}: expected dtype torch.bfloat16 or torch.float16, got {t.dtype}")
    return _lib.IMAGE_F16 if t.dtype == torch.float16 else _lib.IMAGE_BF16


def _fp32_or_bf16(t: torch.Tensor, who: Optional[str]):
    """``(dtype, the C ABI's dtype code)`` of an fp32 or bf16 tensor.  Any other dtype is a ``TypeError`` in the name of
    ``who``; with ``who`` None it passes as fp32, for the per-tensor checks that follow to refuse by the tensor's name."""
    if t.dtype == torch.bfloat16:
        return torch.bfloat16, _lib.DTYPE_BF16
    if t.dtype != torch.float32 and who is not None:
        raise TypeError(f"{who} supports fp32 and bf16, got {t.dtype}")
    return torch.float32, _lib.DTYPE_F32


def half_image_rho_bound(rho: torch.Tensor, D: int) -> torch.Tensor:
    """A rigorous (loose) residual bound of the HALF image from the bf16 residual norms ``rho``, for one-shot callers that
    hold a half image without its ``rho16``: every element that stays normal is rounded to a grid that contains the
    bf16 grid (error <= the bf16 error), every element stored as 0 errs by less than 2^-14, so
    ``rho16 <= rho + sqrt(D) 2^-14``.  Owners of an image keep the measured ``rho16`` instead."""
    return rho + float(D) ** 0.5 * 2.0 ** -14 * 1.001


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def lib():
    return _lib.load()


# ---------------------------------------------------------------------------------------
# neurons
# ---------------------------------------------------------------------------------------

def izh_run_nt(I, spikes, v, u, a, b, c, d, dt) -> None:
    """I, spikes: [N, T] fp32; v, u: [N] fp32 (updated in place)."""
    _need(I, "I", torch.float32); _need(spikes, "spikes", torch.float32)
    _need(v, "v", torch.float32); _need(u, "u", torch.float32)
    N, T = I.shape
    if spikes.shape != I.shape or v.numel() != N or u.numel() != N:
        raise ValueError("izh_run_nt: shape mismatch")
    check(lib().aura_izh_run_nt(_p(I), _p(spikes), _p(v), _p(u), a, b, c, d, dt, N, T, _stream()),
          "aura_izh_run_nt")


def izh_run_btd(I, spikes, v, u, a, b, c, d, dt) -> None:
    """I, spikes: [B, T, D] fp32; v, u: [B*D] fp32 indexed b*D+d."""
    _need(I, "I", torch.float32); _need(spikes, "spikes", torch.float32)
    _need(v, "v", torch.float32); _need(u, "u", torch.float32)
    B, T, D = I.shape
    if spikes.shape != I.shape or v.numel() != B * D or u.numel() != B * D:
        raise ValueError("izh_run_btd: shape mismatch")
    check(lib().aura_izh_run_btd(_p(I), _p(spikes), _p(v), _p(u), a, b, c, d, dt, B, T, D,
                                 _stream()), "aura_izh_run_btd")


def _adex_params(params: Sequence[float]):
    if len(params) != 11:
        raise ValueError("AdEx needs 11 parameters")
    return (ctypes.c_float * 11)(*[float(x) for x in params])


def adex_run_nt(I, spikes, V, w, params: Sequence[float]) -> None:
    _need(I, "I", torch.float32); _need(spikes, "spikes", torch.float32)
    _need(V, "V", torch.float32); _need(w, "w", torch.float32)
    N, T = I.shape
    if spikes.shape != I.shape or V.numel() != N or w.numel() != N:
        raise ValueError("adex_run_nt: shape mismatch")
    arr = _adex_params(params)
    check(lib().aura_adex_run_nt(_p(I), _p(spikes), _p(V), _p(w), ctypes.addressof(arr), N, T,
                                 _stream()), "aura_adex_run_nt")


def adex_run_btd(I, spikes, V, w, params: Sequence[float]) -> None:
    _need(I, "I", torch.float32); _need(spikes, "spikes", torch.float32)
    _need(V, "V", torch.float32); _need(w, "w", torch.float32)
    B, T, D = I.shape
    if spikes.shape != I.shape or V.numel() != B * D or w.numel() != B * D:
        raise ValueError("adex_run_btd: shape mismatch")
    arr = _adex_params(params)
    check(lib().aura_adex_run_btd(_p(I), _p(spikes), _p(V), _p(w), ctypes.addressof(arr), B, T, D,
                                  _stream()), "aura_adex_run_btd")


def lif_run(x, spikes, mem, beta, threshold) -> None:
    """x, spikes: [B, T, size]; mem: [B, size] in/out; beta, threshold: [size].  fp32, or all five bf16 (a
    module moved to bf16: every op rounds to bf16)."""
    dt, code = _fp32_or_bf16(x, "lif_run")
    for t, n in ((x, "x"), (spikes, "spikes"), (mem, "mem"), (beta, "beta"), (threshold, "threshold")):
        _need(t, n, dt)
    B, T, size = x.shape
    if spikes.shape != x.shape or mem.shape != (B, size) or beta.numel() != size or \
            threshold.numel() != size:
        raise ValueError("lif_run: shape mismatch")
    check(lib().aura_lif_run(_p(x), _p(spikes), _p(mem), _p(beta), _p(threshold), B, T, size, code, _stream()),
          "aura_lif_run")


def gif_run(h, out, v, theta, decay: float, L: int, alpha: float, threshold: float, T: int,
            time_invariant: bool = False, mean_out: bool = False) -> None:
    """h: [rows, T, H] (or [rows, H] if time_invariant); out: [rows, T, H] (or [rows, H] if
    mean_out); v, theta: [rows, H] in/out.  fp32 or bf16 (all four the same dtype)."""
    dt, code = _fp32_or_bf16(h, "gif_run")
    for t, n in ((h, "h"), (out, "out"), (v, "v"), (theta, "theta")):
        _need(t, n, dt)
    rows, H = v.shape
    if theta.shape != v.shape:
        raise ValueError("gif_run: v/theta shape mismatch")
    if tuple(h.shape) != ((rows, H) if time_invariant else (rows, T, H)):
        raise ValueError(f"gif_run: h has shape {tuple(h.shape)}")
    if tuple(out.shape) != ((rows, H) if mean_out else (rows, T, H)):
        raise ValueError(f"gif_run: out has shape {tuple(out.shape)}")
    flags = (_lib.GIF_TIME_INVARIANT if time_invariant else 0) | (_lib.GIF_MEAN_OUT if mean_out else 0)
    check(lib().aura_gif_run(_p(h), _p(out), _p(v), _p(theta), decay, int(L), alpha, threshold,
                             rows, T, H, code, flags, _stream()), "aura_gif_run")


# ---------------------------------------------------------------------------------------
# timestep STDP (the rule: include/aura_hip.h, "STDP")
# ---------------------------------------------------------------------------------------

def _stdp_shapes(pre, post, x_trace, y_trace, weight, dw_out, pre_time_invariant: bool):
    """Shape, dtype and contiguity checks of ``stdp_update`` (``ValueError``): ``(B, T, I, O)``.  Touches no device."""
    named = (("pre", pre), ("post", post), ("x_trace", x_trace), ("y_trace", y_trace), ("weight", weight),
             ("dw_out", dw_out))
    for n, t in named:
        if t is not None and not isinstance(t, torch.Tensor):
            raise TypeError(f"stdp_update: {n} must be a torch.Tensor, got {type(t)}")
    if pre is None or post is None:
        raise ValueError("stdp_update: pre and post are required")
    if post.dim() != 3:
        raise ValueError(f"stdp_update: post must be [B, T, O], got {tuple(post.shape)}")
    if pre.dim() != (2 if pre_time_invariant else 3):
        raise ValueError(f"stdp_update: pre must be {'[B, I]' if pre_time_invariant else '[B, T, I]'}, "
                         f"got {tuple(pre.shape)}")
    B, T, O = post.shape
    I = pre.shape[-1]
    if pre.shape[0] != B or (not pre_time_invariant and pre.shape[1] != T):
        raise ValueError(f"stdp_update: pre {tuple(pre.shape)} and post {tuple(post.shape)} disagree in B or T")
    if B < 1 or T < 1:
        raise ValueError("stdp_update: B and T must be at least 1")
    if pre.dtype != post.dtype or pre.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"stdp_update: pre and post share one dtype, fp32 or bf16; got {pre.dtype} and {post.dtype}")
    if I < 4 or O < 4 or I % 4 or O % 4:
        raise ValueError(f"stdp_update: I={I} and O={O} must be multiples of 4")
    for n, t, shape in (("x_trace", x_trace, (B, I)), ("y_trace", y_trace, (B, O)), ("weight", weight, (O, I)),
                        ("dw_out", dw_out, (O, I))):
        if t is None:
            continue
        if t.dtype != torch.float32:
            raise ValueError(f"stdp_update: {n} must be fp32, got {t.dtype}")
        if tuple(t.shape) != shape:
            raise ValueError(f"stdp_update: {n} must be {shape}, got {tuple(t.shape)}")
    if weight is None and dw_out is None:
        raise ValueError("stdp_update: give weight (applied in place), dw_out (dW only), or both")
    for n, t in named:
        if t is not None and not t.is_contiguous():
            raise ValueError(f"stdp_update: {n} must be contiguous")
    return B, T, I, O


def stdp_update(pre, post, x_trace, y_trace, weight=None, dw_out=None, *, lambda_pre: float, lambda_post: float,
                a_plus: float, a_minus: float, lr: float, w_min: float, w_max: float,
                pre_time_invariant: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """Timestep STDP of one dense synapse in one fused launch plus a small reduction (the rule: ``include/aura_hip.h``,
    "STDP").  ``pre`` [B, T, I] (or [B, I] with ``pre_time_invariant``: the same value at every step) and ``post``
    [B, T, O] share one dtype, fp32 or bf16; neither is written.  ``x_trace`` [B, I] / ``y_trace`` [B, O] fp32 are the
    incoming traces (``None``: zero) and are not written either: the traces after the last step are RETURNED as new
    tensors ``(x, y)``.  ``weight`` [O, I] fp32 is updated in place, ``clamp(W + lr dW, w_min, w_max)``; ``dw_out``
    [O, I] fp32 receives dW (with ``weight`` given: the dW that was applied; alone: nothing is applied).  The result is
    a function of the arguments alone: the same call gives the same bits.  No host sync."""
    B, T, I, O = _stdp_shapes(pre, post, x_trace, y_trace, weight, dw_out, pre_time_invariant)
    if weight is not None and not (float(w_min) <= float(w_max)):
        raise ValueError(f"stdp_update: w_min={w_min} must not exceed w_max={w_max}")
    _need(pre, "pre"); _need(post, "post")
    for n, t in (("x_trace", x_trace), ("y_trace", y_trace), ("weight", weight), ("dw_out", dw_out)):
        if t is not None:
            _need(t, n, torch.float32)
            if t.device != pre.device:
                raise ValueError("stdp_update: tensors are on different devices")
    if post.device != pre.device:
        raise ValueError("stdp_update: tensors are on different devices")
    L = lib()
    nbytes = int(L.aura_stdp_workspace_bytes(B, T, I, O))
    if nbytes < 0:
        raise ValueError(f"stdp_update: unsupported shape B={B} T={T} I={I} O={O}")
    x_new = torch.empty(B, I, dtype=torch.float32, device=pre.device)
    y_new = torch.empty(B, O, dtype=torch.float32, device=pre.device)
    flags = (_lib.STDP_PRE_TIME_INVARIANT if pre_time_invariant else 0) | (_lib.STDP_NO_APPLY if weight is None else 0)
    ws = _workspace(pre.device, nbytes)
    check(L.aura_stdp_update(_p(pre), _p(post), _p(x_trace), _p(y_trace), _p(x_new), _p(y_new), _p(weight),
                             _p(dw_out), float(lambda_pre), float(lambda_post), float(a_plus), float(a_minus),
                             float(lr), float(w_min), float(w_max), B, T, I, O,
                             _lib.DTYPE_F32 if pre.dtype == torch.float32 else _lib.DTYPE_BF16, flags, ws, nbytes,
                             _stream()), "aura_stdp_update")
    return x_new, y_new


# ---------------------------------------------------------------------------------------
# place-cell code (the rule: include/aura_hip.h, "Place code")
# ---------------------------------------------------------------------------------------

PLACE_MAX_K, PLACE_MAX_CELLS = 256, 8192


def _place_fp32(who: str, named, what: str = "the place code runs") -> None:
    for n, t in named:
        if t is None:
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{who}: {n} must be a torch.Tensor, got {type(t)}")
        if t.dtype != torch.float32:
            raise TypeError(f"{who}: {n} is {t.dtype}; {what} in fp32 only (fp32 is the limit: "
                            f"bf16 and fp16 are not supported)")
        if not t.is_contiguous():
            raise ValueError(f"{who}: {n} must be contiguous")


def _place_limits(who: str, N: int, P: int, D: int, k) -> int:
    if isinstance(k, bool) or not isinstance(k, int):
        raise TypeError(f"{who}: k must be an int, got {type(k)}")
    if P > PLACE_MAX_CELLS:
        raise ValueError(f"{who}: P={P} cells exceed the limit of {PLACE_MAX_CELLS}")
    if not 1 <= k <= min(P, PLACE_MAX_K):
        raise ValueError(f"{who}: k={k} must be in [1, min(P, {PLACE_MAX_K})] with P={P}")
    if D < 1:
        raise ValueError(f"{who}: D={D} must be at least 1")
    if N > 0x7fffffff:
        raise ValueError(f"{who}: N={N} rows exceed 2^31 - 1")
    return k


def _place_shapes(z, e, w2t, b2, k) -> Tuple[int, int, int, int]:
    """Type, shape and limit checks of ``place_code``: ``(N, P, D, k)``.  Touches no device."""
    _place_fp32("place_code", (("z", z), ("e", e), ("w2t", w2t), ("b2", b2)))
    for n, t in (("z", z), ("e", e), ("w2t", w2t), ("b2", b2)):
        if t is None:
            raise ValueError(f"place_code: {n} is required")
    if z.dim() != 2 or e.dim() != 2 or w2t.dim() != 2 or b2.dim() != 1:
        raise ValueError(f"place_code: z [N, P], e [N, D], w2t [P, D], b2 [D]; got {tuple(z.shape)}, "
                         f"{tuple(e.shape)}, {tuple(w2t.shape)}, {tuple(b2.shape)}")
    N, P = z.shape
    D = e.shape[1]
    if e.shape[0] != N or tuple(w2t.shape) != (P, D) or b2.shape[0] != D:
        raise ValueError(f"place_code: z {tuple(z.shape)}, e {tuple(e.shape)}, w2t {tuple(w2t.shape)} and b2 "
                         f"{tuple(b2.shape)} disagree")
    return N, P, D, _place_limits("place_code", N, P, D, k)


def place_code(z, e, w2t, b2, k: int, dense: bool = True):
    """The sparse place-cell code in one launch (the rule: ``include/aura_hip.h``, "Place code").  ``z`` [N, P] logits,
    ``e`` [N, D] embeddings, ``w2t`` [P, D] the transpose of ``place_to_semantic.weight``, ``b2`` [D]; fp32, contiguous.
    Returns ``(out [N, D], idx [N, k] int32, act [N, k], dense [N, P] or None)``: the exact top ``k`` cells of every row
    (ties to the lower cell, NaN first) in ascending cell index, their sigmoid, ``e + 0.1 (act @ w2t[idx] + b2)`` and,
    with ``dense``, the code scattered into zeros.  A row's bits depend on that row alone.  No host sync."""
    N, P, D, k = _place_shapes(z, e, w2t, b2, k)
    for n, t in (("z", z), ("e", e), ("w2t", w2t), ("b2", b2)):
        _need(t, n, torch.float32)
        if t.device != z.device:
            raise ValueError("place_code: tensors are on different devices")
    dev = z.device
    out = torch.empty(N, D, dtype=torch.float32, device=dev)
    idx = torch.empty(N, k, dtype=torch.int32, device=dev)
    act = torch.empty(N, k, dtype=torch.float32, device=dev)
    code = torch.empty(N, P, dtype=torch.float32, device=dev) if dense else None
    check(lib().aura_place_code(_p(z), _p(e), _p(w2t), _p(b2), N, P, D, k, _p(idx), _p(act), _p(out), _p(code),
                                _stream()), "aura_place_code")
    return out, idx, act, code


def _place_backward_shapes(g_out, g_dense, idx, act, w2t) -> Tuple[int, int, int, int]:
    _place_fp32("place_code_backward", (("g_out", g_out), ("g_dense", g_dense), ("act", act), ("w2t", w2t)))
    for n, t in (("g_out", g_out), ("idx", idx), ("act", act), ("w2t", w2t)):
        if t is None:
            raise ValueError(f"place_code_backward: {n} is required")
    if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int32:
        raise TypeError("place_code_backward: idx must be an int32 tensor")
    if not idx.is_contiguous():
        raise ValueError("place_code_backward: idx must be contiguous")
    if g_out.dim() != 2 or idx.dim() != 2 or w2t.dim() != 2:
        raise ValueError("place_code_backward: g_out [N, D], idx [N, k], act [N, k], w2t [P, D]")
    N, D = g_out.shape
    P = w2t.shape[0]
    k = idx.shape[1]
    if idx.shape[0] != N or act.shape != idx.shape or w2t.shape[1] != D:
        raise ValueError(f"place_code_backward: g_out {tuple(g_out.shape)}, idx {tuple(idx.shape)}, act "
                         f"{tuple(act.shape)} and w2t {tuple(w2t.shape)} disagree")
    if g_dense is not None and tuple(g_dense.shape) != (N, P):
        raise ValueError(f"place_code_backward: g_dense must be {(N, P)}, got {tuple(g_dense.shape)}")
    return N, P, D, _place_limits("place_code_backward", N, P, D, int(k))


def place_code_backward(g_out, g_dense, idx, act, w2t) -> torch.Tensor:
    """The logit gradient of ``place_code`` in one launch: ``g_z`` [N, P], ``(0.1 <g_out[n], w2t[j]> + g_dense[n, j])
    act (1 - act)`` at the winners and +0.0 elsewhere.  ``g_dense`` may be ``None``; ``idx`` / ``act`` are what the
    forward returned.  The dot products have a fixed order: the same call gives the same bits."""
    N, P, D, k = _place_backward_shapes(g_out, g_dense, idx, act, w2t)
    for n, t in (("g_out", g_out), ("g_dense", g_dense), ("idx", idx), ("act", act), ("w2t", w2t)):
        if t is not None:
            _need(t, n)
            if t.device != g_out.device:
                raise ValueError("place_code_backward: tensors are on different devices")
    g_z = torch.empty(N, P, dtype=torch.float32, device=g_out.device)
    check(lib().aura_place_code_backward(_p(g_out), _p(g_dense), _p(idx), _p(act), _p(w2t), N, P, D, k, _p(g_z),
                                         _stream()), "aura_place_code_backward")
    return g_z


class PlaceCodeFunction(torch.autograd.Function):
    """``(z, e, w2t, b2) -> (out, idx, act, dense or None)`` with gradients for all four inputs.  ``g_z`` is the mirror
    launch; ``g_e = g_out``, ``g_b2 = 0.1 sum_n g_out`` and ``g_w2t = 0.1 dense^T g_out`` are library calls (the last a
    GEMM over the dense code, rebuilt from idx / act when the forward did not write it).  ``idx`` carries no gradient;
    a gradient that reaches ``act`` is folded into the winners' cells like one that reaches ``dense``.  ``weight``
    [D, P]: the parameter that a detached ``w2t`` is the transpose of; its gradient is then ``0.1 g_out^T dense`` and
    ``w2t`` gets none (the module's cached transpose)."""

    @staticmethod
    def forward(ctx, z, e, w2t, b2, k: int, want_dense: bool, weight=None):
        out, idx, act, code = place_code(z, e, w2t, b2, k, dense=want_dense)
        ctx.save_for_backward(idx, act, w2t, code)
        ctx.n_cells = z.shape[1]
        ctx.mark_non_differentiable(idx)
        return out, idx, act, code

    @staticmethod
    def backward(ctx, g_out, _g_idx, g_act, g_code):
        idx, act, w2t, code = ctx.saved_tensors
        N, k = idx.shape
        P = ctx.n_cells
        if g_out is None:
            g_out = torch.zeros(N, w2t.shape[1], dtype=torch.float32, device=idx.device)
        g_out = g_out.contiguous()
        if g_act is not None:
            spread = torch.zeros(N, P, dtype=torch.float32, device=idx.device).scatter_(1, idx.long(), g_act)
            g_code = spread if g_code is None else g_code + spread
        g_z = g_e = g_w2t = g_b2 = g_weight = None
        if ctx.needs_input_grad[0]:
            g_z = place_code_backward(g_out, None if g_code is None else g_code.contiguous(), idx, act, w2t)
        if ctx.needs_input_grad[1]:
            g_e = g_out
        if (ctx.needs_input_grad[2] or ctx.needs_input_grad[6]) and code is None:
            code = torch.zeros(N, P, dtype=torch.float32, device=idx.device).scatter_(1, idx.long(), act)
        if ctx.needs_input_grad[2]:
            g_w2t = 0.1 * (code.t() @ g_out)
        if ctx.needs_input_grad[6]:
            g_weight = 0.1 * (g_out.t() @ code)
        if ctx.needs_input_grad[3]:
            g_b2 = 0.1 * g_out.sum(0)
        return g_z, g_e, g_w2t, g_b2, None, None, g_weight


# ---------------------------------------------------------------------------------------
# theta-gamma positions (the rule: include/aura_hip.h, "Theta-gamma")
# ---------------------------------------------------------------------------------------

THETA_MAX_D = 2048


def _theta_fp32(who: str, named) -> None:
    _place_fp32(who, named, "the theta-gamma kernels run")


def _theta_required(who: str, named) -> None:
    for n, t in named:
        if t is None:
            raise ValueError(f"{who}: {n} is required")


def _theta_device(who: str, named, wide=()) -> torch.device:
    """Every tensor on one HIP device; the ``wide`` ones ([.., D] rows, which move as float4 when D % 4 == 0) 16-byte
    aligned.  After the shape checks."""
    dev = None
    for n, t in named:
        if t is None:
            continue
        _need(t, f"{who}: {n}")
        dev = t.device if dev is None else dev
        if t.device != dev:
            raise ValueError(f"{who}: tensors are on different devices")
        if n in wide and t.shape[-1] % 4 == 0 and t.data_ptr() % 16:
            raise ValueError(f"{who}: {n} is not 16-byte aligned (a view into the middle of a buffer?)")
    return dev


def theta_gamma_ratio(theta_freq: float, gamma_freq: float) -> float:
    """The rule's ``ratio``: ``fp32(double(gamma_freq) / double(theta_freq))``."""
    theta_freq, gamma_freq = float(theta_freq), float(gamma_freq)
    if not (theta_freq == theta_freq and gamma_freq == gamma_freq) or theta_freq == 0.0:
        raise ValueError(f"theta_gamma: theta_freq={theta_freq} and gamma_freq={gamma_freq} give no frequency ratio")
    return float(np.float32(gamma_freq / theta_freq))


def _theta_table_shapes(theta_off, gamma_off, amp, max_seq_len, positions, start, rows) -> Tuple[int, int]:
    """Type, shape and limit checks of ``theta_gamma_table``: ``(R, D)``.  Touches no device."""
    who = "theta_gamma_table"
    named = (("theta_off", theta_off), ("gamma_off", gamma_off), ("amp", amp))
    _theta_required(who, named)
    _theta_fp32(who, named + (("positions", positions),))
    if theta_off.dim() != 1 or gamma_off.shape != theta_off.shape or amp.shape != theta_off.shape:
        raise ValueError(f"{who}: theta_off, gamma_off and amp are [D]; got {tuple(theta_off.shape)}, "
                         f"{tuple(gamma_off.shape)}, {tuple(amp.shape)}")
    D = theta_off.shape[0]
    if not 1 <= D <= THETA_MAX_D:
        raise ValueError(f"{who}: D={D} must be in [1, {THETA_MAX_D}]")
    if isinstance(max_seq_len, bool) or not isinstance(max_seq_len, int) or max_seq_len < 1:
        raise ValueError(f"{who}: max_seq_len={max_seq_len!r} must be an int of at least 1")
    if positions is not None:
        if rows is not None or start != 0:
            raise ValueError(f"{who}: give positions, or start and rows, not both")
        if positions.dim() != 1:
            raise ValueError(f"{who}: positions is [R] fp32, got {tuple(positions.shape)}")
        R = positions.shape[0]
    else:
        if rows is None:
            raise ValueError(f"{who}: give positions, or start and rows")
        for n, v in (("start", start), ("rows", rows)):
            if isinstance(v, bool) or not isinstance(v, int):
                raise TypeError(f"{who}: {n} must be an int, got {type(v)}")
        if rows < 0 or not -2 ** 62 <= start <= 2 ** 62:
            raise ValueError(f"{who}: rows={rows} must not be negative (start={start})")
        R = rows
    if R > 0x7fffffff:
        raise ValueError(f"{who}: R={R} rows exceed 2^31 - 1")
    return R, D


def theta_gamma_table(theta_off, gamma_off, amp, max_seq_len: int, ratio: float, positions=None, start: int = 0,
                      rows: Optional[int] = None, derivatives: bool = False, pe: bool = True):
    """The phase-code table in one launch (the rule: ``include/aura_hip.h``, "Theta-gamma"): ``pe`` [R, D] for the fp32
    ``positions`` [R], or for ``start, start + 1, ..`` (``rows`` of them, formed in the kernel) when ``positions`` is
    ``None``.  With ``derivatives`` returns ``(pe, d_theta, d_gamma, d_amp)``, each [R, D]; ``pe=False`` leaves the
    first ``None`` and unwritten.  The only place the sines and cosines are evaluated.  No host sync."""
    R, D = _theta_table_shapes(theta_off, gamma_off, amp, max_seq_len, positions, start, rows)
    if not (derivatives or pe):
        raise ValueError("theta_gamma_table: nothing to compute")
    ratio = float(ratio)
    dev = _theta_device("theta_gamma_table", (("theta_off", theta_off), ("gamma_off", gamma_off), ("amp", amp),
                                              ("positions", positions)))
    new = lambda: torch.empty(R, D, dtype=torch.float32, device=dev)
    out = new() if pe else None
    d = (new(), new(), new()) if derivatives else (None, None, None)
    check(lib().aura_theta_gamma_table(_p(positions), start, R, D, _p(theta_off), _p(gamma_off), _p(amp), max_seq_len,
                                       ratio, _p(out), _p(d[0]), _p(d[1]), _p(d[2]), _stream()),
          "aura_theta_gamma_table")
    return (out, *d) if derivatives else out


def _theta_norm_shapes(who: str, x, table, w, b, seq_len, eps=1e-5) -> Tuple[int, int, int, int]:
    """``(N, S, R, D)`` of a fused call.  Touches no device."""
    named = (("x", x), ("table", table), ("w", w)) + ((("b", b),) if who == "theta_gamma_norm" else ())
    _theta_required(who, named)
    _theta_fp32(who, named)
    if x.dim() != 2 or table.dim() != 2 or w.dim() != 1 or (b is not None and b.dim() != 1):
        raise ValueError(f"{who}: x [N, D], table [R, D], w [D], b [D]; got {tuple(x.shape)}, {tuple(table.shape)}, "
                         f"{tuple(w.shape)}" + ("" if b is None else f", {tuple(b.shape)}"))
    N, D = x.shape
    R = table.shape[0]
    if table.shape[1] != D or w.shape[0] != D or (b is not None and b.shape[0] != D):
        raise ValueError(f"{who}: x {tuple(x.shape)}, table {tuple(table.shape)}, w {tuple(w.shape)}"
                         + ("" if b is None else f", b {tuple(b.shape)}") + " disagree in D")
    if not 1 <= D <= THETA_MAX_D:
        raise ValueError(f"{who}: D={D} must be in [1, {THETA_MAX_D}]")
    if N > 0x7fffffff:
        raise ValueError(f"{who}: N={N} tokens exceed 2^31 - 1")
    if isinstance(seq_len, bool) or not isinstance(seq_len, int) or seq_len < 1:
        raise ValueError(f"{who}: seq_len={seq_len!r} must be an int of at least 1")
    if not (R == N or (R == seq_len and N % seq_len == 0)):
        raise ValueError(f"{who}: a table of {R} rows fits neither the {N} tokens (one row each) nor sequences of "
                         f"seq_len={seq_len} (shared rows, N a multiple of it)")
    if not isinstance(eps, float) or not eps >= 0.0:
        raise ValueError(f"{who}: eps={eps!r} must be a float that is not negative")
    return N, seq_len, R, D


def theta_gamma_norm(x, table, w, b, seq_len: int, eps: float = 1e-5):
    """``LayerNorm(x + pe)`` in one launch: ``x`` [N, D] the tokens of sequences of ``seq_len``, ``table`` [R, D] from
    ``theta_gamma_table`` with R = ``seq_len`` (token n reads row ``n % seq_len``) or R = N (row n), ``w`` / ``b`` [D]
    the norm's weight and bias.  Returns ``(y [N, D], mean [N], rstd [N])``; ``x + pe`` is never written.  A token's
    bits are the same alone and in any batch.  No host sync."""
    N, S, R, D = _theta_norm_shapes("theta_gamma_norm", x, table, w, b, seq_len, eps)
    dev = _theta_device("theta_gamma_norm", (("x", x), ("table", table), ("w", w), ("b", b)),
                        wide=("x", "table", "w", "b"))
    y = torch.empty(N, D, dtype=torch.float32, device=dev)
    mean = torch.empty(N, dtype=torch.float32, device=dev)
    rstd = torch.empty(N, dtype=torch.float32, device=dev)
    check(lib().aura_theta_gamma_norm(_p(x), _p(table), _p(w), _p(b), eps, N, S, R, D, _p(y), _p(mean), _p(rstd),
                                      _stream()), "aura_theta_gamma_norm")
    return y, mean, rstd


def theta_gamma_groups(N: int) -> int:
    """How many partial rows the backward adds per column: ``clamp(ceil(N / 16), 1, 1024)`` (the header's G)."""
    return max(1, min(1024, -(-int(N) // 16)))


def _theta_backward_shapes(g_y, x, table, derivs, mean, rstd, w, seq_len) -> Tuple[int, int, int, int]:
    who = "theta_gamma_norm_backward"
    N, S, R, D = _theta_norm_shapes(who, x, table, w, None, seq_len)
    named = (("g_y", g_y), ("mean", mean), ("rstd", rstd))
    _theta_required(who, named)
    _theta_fp32(who, named)
    if tuple(g_y.shape) != (N, D):
        raise ValueError(f"{who}: g_y must be {(N, D)}, got {tuple(g_y.shape)}")
    if tuple(mean.shape) != (N,) or tuple(rstd.shape) != (N,):
        raise ValueError(f"{who}: mean and rstd must be {(N,)}, got {tuple(mean.shape)} and {tuple(rstd.shape)}")
    if derivs is not None:
        if not isinstance(derivs, (tuple, list)) or len(derivs) != 3:
            raise ValueError(f"{who}: derivatives is (d_theta, d_gamma, d_amp) or None")
        named = tuple(zip(("d_theta", "d_gamma", "d_amp"), derivs))
        _theta_required(who, named)
        _theta_fp32(who, named)
        for n, t in named:
            if tuple(t.shape) != (R, D):
                raise ValueError(f"{who}: {n} must be {(R, D)} like the table, got {tuple(t.shape)}")
    return N, S, R, D


def theta_gamma_norm_backward(g_y, x, table, derivatives, mean, rstd, w, seq_len: int, column_sums: bool = True):
    """The backward of ``theta_gamma_norm``: ``(g_x [N, D], grads)``.  ``derivatives`` is ``(d_theta, d_gamma, d_amp)``
    from ``theta_gamma_table(.., derivatives=True)`` or ``None``; ``mean`` / ``rstd`` are what the forward returned.
    ``grads`` is [5, D] -- ``g_w, g_b, g_theta, g_gamma, g_amp`` -- with the derivatives, [2, D] without them, and
    ``None`` with ``column_sums=False`` (one launch instead of two; not with derivatives).  Every sum has a fixed order:
    the same call gives the same bits."""
    N, S, R, D = _theta_backward_shapes(g_y, x, table, derivatives, mean, rstd, w, seq_len)
    if derivatives is not None and not column_sums:
        raise ValueError("theta_gamma_norm_backward: derivative tables are read for the column sums only")
    d = tuple(derivatives) if derivatives is not None else (None, None, None)
    dev = _theta_device("theta_gamma_norm_backward", (("g_y", g_y), ("x", x), ("table", table), ("d_theta", d[0]),
                                                      ("d_gamma", d[1]), ("d_amp", d[2]), ("mean", mean),
                                                      ("rstd", rstd), ("w", w)),
                        wide=("g_y", "x", "table", "d_theta", "d_gamma", "d_amp", "w"))
    g_x = torch.empty(N, D, dtype=torch.float32, device=dev)
    partials = grads = None
    if column_sums:
        partials = torch.empty(theta_gamma_groups(N), 5, D, dtype=torch.float32, device=dev)
        grads = torch.zeros(5, D, dtype=torch.float32, device=dev)      # N == 0 launches nothing: the sums are zero
    check(lib().aura_theta_gamma_norm_backward(_p(g_y), _p(x), _p(table), _p(d[0]), _p(d[1]), _p(d[2]), _p(mean),
                                               _p(rstd), _p(w), N, S, R, D, _p(g_x), _p(partials), _p(grads),
                                               _stream()), "aura_theta_gamma_norm_backward")
    if grads is not None and derivatives is None:
        grads = grads[:2]
    return g_x, grads


class ThetaGammaNormFunction(torch.autograd.Function):
    """``(x, table, theta_off, gamma_off, amp, w, b) -> LayerNorm(x + pe)`` with gradients for all but ``table``, which
    is the detached ``theta_gamma_table`` of the three parameters at ``geometry = (positions or None, start,
    max_seq_len, ratio)``.  Saves ``x``, the table, ``mean`` and ``rstd`` (never ``x + pe``); the derivative tables are
    built in backward by a second table call, and only when one of the three parameters wants a gradient.  Without any
    parameter gradient the backward is one launch."""

    @staticmethod
    def forward(ctx, x, table, theta_off, gamma_off, amp, w, b, seq_len: int, eps: float, geometry):
        y, mean, rstd = theta_gamma_norm(x, table, w, b, seq_len, eps)
        positions = geometry[0]
        ctx.save_for_backward(x, table, mean, rstd, theta_off, gamma_off, amp, w, positions)
        ctx.seq_len, ctx.geometry = seq_len, geometry[1:]
        return y

    @staticmethod
    def backward(ctx, g_y):
        x, table, mean, rstd, theta_off, gamma_off, amp, w, positions = ctx.saved_tensors
        start, max_seq_len, ratio = ctx.geometry
        need = ctx.needs_input_grad
        phase, affine = any(need[2:5]), any(need[5:7])
        if not (need[0] or phase or affine):
            return (None,) * 10
        derivs = None
        if phase:
            rows = None if positions is not None else table.shape[0]
            derivs = theta_gamma_table(theta_off, gamma_off, amp, max_seq_len, ratio, positions=positions, start=start,
                                       rows=rows, derivatives=True, pe=False)[1:]
        g_x, grads = theta_gamma_norm_backward(g_y.contiguous(), x, table, derivs, mean, rstd, w, ctx.seq_len,
                                               column_sums=phase or affine)
        pick = lambda i, k: grads[k] if need[i] else None
        return (g_x if need[0] else None, None, *(pick(2 + k, 2 + k) if phase else None for k in range(3)),
                pick(5, 0) if affine else None, pick(6, 1) if affine else None, None, None, None)


# ---------------------------------------------------------------------------------------
# prosody attention (the rule: include/aura_hip.h, "Prosody attention")
# ---------------------------------------------------------------------------------------

PROSODY_MAX_S, PROSODY_MAX_K, PROSODY_MAX_SMOOTHING, PROSODY_MAX_ID = 8192, 256, 64, 1 << 24


class ProsodyAttention:
    """What ``prosody_attention`` returns: ``gains`` and ``salience`` [B, S], ``mu`` [B], ``winners`` [B, k] int32 in
    rank order (-1 beyond ``min(k, len)``), ``state`` [B, 3] (the membranes after the last live step), and, when asked
    for, ``spikes`` and ``channels`` [3, B, S] (amp, pitch, boundary), else ``None``."""
    __slots__ = ("gains", "salience", "mu", "winners", "state", "spikes", "channels")

    def __init__(self, gains, salience, mu, winners, state, spikes=None, channels=None):
        self.gains, self.salience, self.mu, self.winners, self.state = gains, salience, mu, winners, state
        self.spikes, self.channels = spikes, channels


def _prosody_ids(who: str, ids) -> Tuple[int, int]:
    if not isinstance(ids, torch.Tensor):
        raise TypeError(f"{who}: ids must be a torch.Tensor, got {type(ids)}")
    if ids.dtype not in (torch.int64, torch.int32):
        raise TypeError(f"{who}: ids is {ids.dtype}; token ids are int64 or int32")
    if ids.dim() != 2:
        raise ValueError(f"{who}: ids is [B, S], got {tuple(ids.shape)}")
    if not ids.is_contiguous():
        raise ValueError(f"{who}: ids must be contiguous")
    return ids.shape[0], ids.shape[1]


def _prosody_shapes(ids, channels, k, decay, weights, gain_up, min_gain, max_gain, smoothing, lengths,
                    state) -> Tuple[int, int, int, int]:
    """Type, shape and limit checks of ``prosody_attention``: ``(B, S, k, m)``.  Touches no device and reads no
    value."""
    who = "prosody_attention"
    if (ids is None) == (channels is None):
        raise ValueError(f"{who}: give token ids or the three channels, not both and not neither")
    if ids is not None:
        B, S = _prosody_ids(who, ids)
    else:
        if not isinstance(channels, (tuple, list)) or len(channels) != 3:
            raise TypeError(f"{who}: channels is the triple (amp, pitch, boundary)")
        named = tuple(zip(("amp", "pitch", "boundary"), channels))
        _theta_required(who, named)
        _place_fp32(who, named, "prosody attention runs")
        if channels[0].dim() != 2 or any(c.shape != channels[0].shape for c in channels):
            raise ValueError(f"{who}: amp, pitch and boundary are [B, S] alike, got "
                             + ", ".join(str(tuple(c.shape)) for c in channels))
        B, S = channels[0].shape
    if not 1 <= S <= PROSODY_MAX_S:
        raise ValueError(f"{who}: S={S} must be in [1, {PROSODY_MAX_S}]")
    if B > 0x7fffffff:
        raise ValueError(f"{who}: B={B} rows exceed 2^31 - 1")
    for n, v in (("k", k), ("smoothing", smoothing)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError(f"{who}: {n} must be an int, got {type(v)}")
    if not 1 <= k <= min(S, PROSODY_MAX_K):
        raise ValueError(f"{who}: k={k} must be in [1, min(S, {PROSODY_MAX_K})] with S={S}")
    if not 0 <= smoothing <= PROSODY_MAX_SMOOTHING:
        raise ValueError(f"{who}: smoothing={smoothing} must be in [0, {PROSODY_MAX_SMOOTHING}]")
    for n, t in (("decay", decay), ("weights", weights)):
        _theta_required(who, ((n, t),))
        _place_fp32(who, ((n, t),), "prosody attention runs")
        if tuple(t.shape) != (3,):
            raise ValueError(f"{who}: {n} is [3] (amp, pitch, boundary), got {tuple(t.shape)}")
    for n, v in (("gain_up", gain_up), ("min_gain", min_gain), ("max_gain", max_gain)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or abs(v) == float("inf"):
            raise ValueError(f"{who}: {n}={v!r} must be a finite number")
    if lengths is not None:
        if not isinstance(lengths, torch.Tensor) or lengths.dtype != torch.int32:
            raise TypeError(f"{who}: lengths must be an int32 tensor")
        if tuple(lengths.shape) != (B,):
            raise ValueError(f"{who}: lengths is [{B}], got {tuple(lengths.shape)}")
        if not lengths.is_contiguous():
            raise ValueError(f"{who}: lengths must be contiguous")
    if state is not None:
        _place_fp32(who, (("state", state),), "prosody attention runs")
        if tuple(state.shape) != (B, 3):
            raise ValueError(f"{who}: state is [{B}, 3], got {tuple(state.shape)}")
    return B, S, k, max(1, smoothing)


def _prosody_values(who: str, ids, lengths, S: int) -> None:
    """The checks that read values (a host sync on a device tensor): ids in [0, 2^24), lengths in [0, S]."""
    if ids is not None and ids.numel():
        lo, hi = int(ids.min()), int(ids.max())
        if lo < 0 or hi >= PROSODY_MAX_ID:
            raise ValueError(f"{who}: token ids must be in [0, 2^24) (fp32 holds them exactly); got {lo} .. {hi}")
    if lengths is not None and lengths.numel():
        lo, hi = int(lengths.min()), int(lengths.max())
        if lo < 0 or hi > S:
            raise ValueError(f"{who}: lengths must be in [0, S={S}]; got {lo} .. {hi}")


def prosody_attention(ids=None, channels=None, *, k: int, decay, weights, gain_up: float = 1.8,
                      min_gain: float = 0.5, max_gain: float = 2.5, smoothing: int = 0, normalize: bool = True,
                      lengths=None, state=None, want_spikes: bool = False, want_channels: bool = False,
                      validate: bool = True) -> ProsodyAttention:
    """Attention gains from token ids (or from three given prosody channels) in one launch (the rule:
    ``include/aura_hip.h``, "Prosody attention").  ``ids`` [B, S] int64 / int32 in [0, 2^24), or ``channels`` = (amp,
    pitch, boundary), each [B, S] fp32; ``decay`` and ``weights`` [3] fp32 on the device; ``lengths`` [B] int32 (rows
    end there: beyond it spikes and salience are 0 and gains are ``mu``); ``state`` [B, 3] the membranes to start from.
    Forward only.  ``validate`` reads the range of ``ids`` and ``lengths`` before the launch, which waits for the device;
    the kernel itself is safe for any value (an id beyond 2^24 merely loses its low bits, a length is clamped), so a
    caller who knows its vocabulary can switch it off and keep the call asynchronous."""
    who = "prosody_attention"
    B, S, k, m = _prosody_shapes(ids, channels, k, decay, weights, gain_up, min_gain, max_gain, smoothing, lengths,
                                 state)
    named = ((("ids", ids),) if ids is not None else tuple(zip(("amp", "pitch", "boundary"), channels))) + (
        ("decay", decay), ("weights", weights), ("lengths", lengths), ("state", state))
    if validate:
        _prosody_values(who, ids, lengths, S)
    dev = _theta_device(who, named)
    f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    out = ProsodyAttention(f32(B, S), f32(B, S), f32(B), torch.empty(B, k, dtype=torch.int32, device=dev), f32(B, 3),
                           f32(3, B, S) if want_spikes else None, f32(3, B, S) if want_channels else None)
    ch = (None, None, None) if ids is not None else channels
    check(lib().aura_prosody_attention(_p(ids), 0 if ids is None else ids.element_size(), _p(ch[0]), _p(ch[1]),
                                       _p(ch[2]), _p(lengths), _p(state), _p(decay), _p(weights), float(gain_up),
                                       float(min_gain), float(max_gain), m, int(bool(normalize)), B, S, k,
                                       _p(out.gains), _p(out.salience), _p(out.mu), _p(out.winners), _p(out.state),
                                       _p(out.spikes), _p(out.channels), _stream()), "aura_prosody_attention")
    return out


def prosody_channels(ids, validate: bool = True) -> torch.Tensor:
    """The three prosody channels of token ids, [3, B, S] fp32 (amp, pitch, boundary): the same launch as
    ``prosody_attention`` with only the channels requested."""
    who = "prosody_channels"
    B, S = _prosody_ids(who, ids)
    if not 1 <= S <= PROSODY_MAX_S:
        raise ValueError(f"{who}: S={S} must be in [1, {PROSODY_MAX_S}]")
    if validate:
        _prosody_values(who, ids, None, S)
    _need(ids, f"{who}: ids")
    out = torch.empty(3, B, S, dtype=torch.float32, device=ids.device)
    check(lib().aura_prosody_attention(_p(ids), ids.element_size(), None, None, None, None, None, None, None, 0.0, 0.0,
                                       0.0, 1, 0, B, S, 1, None, None, None, None, None, None, _p(out), _stream()),
          "aura_prosody_attention")
    return out


# ---------------------------------------------------------------------------------------
# decode attention (the rule: include/aura_hip.h, "Decode attention")
# ---------------------------------------------------------------------------------------

DECODE_CHUNK, DECODE_MAX_D, DECODE_MAX_HEAD, DECODE_MAX_CAP = 256, 2048, 128, 32768


def attn_decode_chunks(capacity: int) -> int:
    """The chunk count that serves every length of a cache of ``capacity`` positions: ``ceil(capacity / 256)``."""
    return -(-int(capacity) // DECODE_CHUNK)


def attn_decode_workspace_floats(B: int, H: int, dh: int, n_chunks: int) -> int:
    """Floats of partials workspace of a step: per (b, h) a header of 4 and ``n_chunks`` chunks of ``4 + dh``."""
    return max(4, B * H * (4 + n_chunks * (4 + dh)))


def _attn_decode_shapes(q, k_new, v_new, x, prosody, Wp, bp, wm, bm, lengths, k_cache, v_cache, workspace,
                        n_chunks) -> Tuple[int, int, int, int, int]:
    """Type, shape and limit checks of ``attn_decode_step``: ``(B, H, dh, cap, n_chunks)``.  Touches no device."""
    who = "attn_decode_step"
    _theta_required(who, (("q", q), ("k_new", k_new), ("v_new", v_new), ("lengths", lengths), ("k_cache", k_cache),
                          ("v_cache", v_cache), ("workspace", workspace)))
    _place_fp32(who, (("q", q), ("k_new", k_new), ("v_new", v_new), ("x", x), ("prosody", prosody), ("Wp", Wp),
                      ("bp", bp), ("wm", wm), ("bm", bm), ("k_cache", k_cache), ("v_cache", v_cache),
                      ("workspace", workspace)), "the decode step runs")
    if not isinstance(lengths, torch.Tensor):
        raise TypeError(f"{who}: lengths must be a torch.Tensor, got {type(lengths)}")
    if lengths.dtype != torch.int32:
        raise TypeError(f"{who}: lengths is {lengths.dtype}; the kernel reads and advances int32 lengths")
    if not lengths.is_contiguous():
        raise ValueError(f"{who}: lengths must be contiguous")
    if k_cache.dim() != 4 or v_cache.shape != k_cache.shape:
        raise ValueError(f"{who}: k_cache and v_cache are [B, H, cap, dh]; got {tuple(k_cache.shape)}, "
                         f"{tuple(v_cache.shape)}")
    B, H, cap, dh = k_cache.shape
    D = H * dh
    if H < 1 or dh % 4 != 0 or not 4 <= dh <= DECODE_MAX_HEAD:
        raise ValueError(f"{who}: dh={dh} must be a multiple of 4 in [4, {DECODE_MAX_HEAD}] (H={H})")
    if D > DECODE_MAX_D:
        raise ValueError(f"{who}: D = H dh = {D} exceeds {DECODE_MAX_D}")
    if not 1 <= cap <= DECODE_MAX_CAP:
        raise ValueError(f"{who}: cap={cap} must be in [1, {DECODE_MAX_CAP}]")
    for n, t in (("q", q), ("k_new", k_new), ("v_new", v_new)):
        if tuple(t.shape) != (B, D):
            raise ValueError(f"{who}: {n} is [B, D] = ({B}, {D}), got {tuple(t.shape)}")
    if tuple(lengths.shape) != (B,):
        raise ValueError(f"{who}: lengths is [B] = ({B},), got {tuple(lengths.shape)}")
    if prosody is not None:
        if tuple(prosody.shape) != (B, 4):
            raise ValueError(f"{who}: prosody is [B, 4] = ({B}, 4), got {tuple(prosody.shape)}")
        _theta_required(who, (("Wp (with prosody)", Wp), ("bp (with prosody)", bp)))
        if tuple(Wp.shape) != (H, 4) or tuple(bp.shape) != (H,):
            raise ValueError(f"{who}: Wp is [H, 4] and bp [H] with H={H}; got {tuple(Wp.shape)}, {tuple(bp.shape)}")
    if (wm is None) != (bm is None):
        raise ValueError(f"{who}: wm and bm are the memory gate's weight and bias: give both or neither")
    if wm is not None:
        _theta_required(who, (("x (with wm)", x),))
        if wm.numel() != D or bm.numel() != 1:
            raise ValueError(f"{who}: wm holds D={D} weights and bm one bias; got {tuple(wm.shape)}, {tuple(bm.shape)}")
        if tuple(x.shape) != (B, D):
            raise ValueError(f"{who}: x is [B, D] = ({B}, {D}), got {tuple(x.shape)}")
    if n_chunks is None:
        n_chunks = attn_decode_chunks(cap)
    if isinstance(n_chunks, bool) or not isinstance(n_chunks, int):
        raise TypeError(f"{who}: n_chunks must be an int, got {type(n_chunks)}")
    if n_chunks < 1 or n_chunks * DECODE_CHUNK > cap + DECODE_CHUNK - 1:
        raise ValueError(f"{who}: n_chunks={n_chunks} must be in [1, ceil(cap / {DECODE_CHUNK})] with cap={cap}")
    if B * H * n_chunks > 0x7fffffff:
        raise ValueError(f"{who}: B H n_chunks = {B * H * n_chunks} waves exceed 2^31 - 1")
    need = attn_decode_workspace_floats(B, H, dh, n_chunks)
    if workspace.numel() < need:
        raise ValueError(f"{who}: workspace holds {workspace.numel()} floats, the step needs {need}")
    return B, H, dh, cap, n_chunks


def attn_decode_step(q, k_new, v_new, x, prosody, Wp, bp, wm, bm, lengths, k_cache, v_cache, workspace,
                     n_chunks: Optional[int] = None, advance: bool = True, return_scale: bool = False):
    """One cached decoding step of HippocampalProsodyAttention in two launches (the rule: ``include/aura_hip.h``,
    "Decode attention"): scales the new query row ``q`` [B, D] by the prosody and memory gates (``prosody`` [B, 4] with
    ``Wp`` [H, 4], ``bp`` [H]; ``wm`` [D], ``bm`` [1] with the normed hidden row ``x`` [B, D]; either may be ``None``),
    appends ``k_new`` / ``v_new`` at position ``lengths[b]`` of ``k_cache`` / ``v_cache`` [B, H, cap, dh], attends over
    positions ``0 .. lengths[b]`` and returns ``ctx`` [B, D] in the layout ``o_proj`` reads.  Rows with a length outside
    ``[0, cap)`` are inactive: zeros, nothing written.  ``advance`` adds one to the active rows' int32 ``lengths`` on the
    device.  ``workspace``: ``attn_decode_workspace_floats`` fp32, owned by the caller.  ``return_scale`` also returns
    the scale ``s`` [B, H].  A row's bits do not depend on the batch, ``cap`` or ``n_chunks``.  No host sync."""
    B, H, dh, cap, n_chunks = _attn_decode_shapes(q, k_new, v_new, x, prosody, Wp, bp, wm, bm, lengths, k_cache,
                                                   v_cache, workspace, n_chunks)
    if prosody is None:
        Wp = bp = None
    if wm is None:
        x = None
    dev = _theta_device("attn_decode_step", (("q", q), ("k_new", k_new), ("v_new", v_new), ("x", x), ("prosody", prosody),
                                             ("Wp", Wp), ("bp", bp), ("wm", wm), ("bm", bm), ("lengths", lengths),
                                             ("k_cache", k_cache), ("v_cache", v_cache), ("workspace", workspace)),
                        wide=("q", "k_new", "v_new", "x", "wm", "k_cache", "v_cache", "workspace"))
    ctx = torch.empty(B, H * dh, dtype=torch.float32, device=dev)
    scale = torch.empty(B, H, dtype=torch.float32, device=dev) if return_scale else None
    check(lib().aura_attn_decode_step(_p(q), _p(k_new), _p(v_new), _p(x), _p(prosody), _p(Wp), _p(bp), _p(wm), _p(bm),
                                      _p(lengths), _p(k_cache), _p(v_cache), B, H, dh, cap, n_chunks, int(bool(advance)),
                                      _p(workspace), workspace.numel() * 4, _p(ctx), _p(scale), _stream()),
          "aura_attn_decode_step")
    return (ctx, scale) if return_scale else ctx


DECODE_EXTEND_MAX = 32


def attn_decode_extend_workspace_floats(B: int, m: int, H: int, dh: int, n_chunks: int) -> int:
    """Floats of partials workspace of an extend of ``m`` tokens: the step's for ``B m`` rows."""
    return attn_decode_workspace_floats(B * m, H, dh, n_chunks)


def _attn_decode_extend_shapes(q, k_new, v_new, x, prosody, Wp, bp, wm, bm, lengths, k_cache, v_cache, workspace,
                               n_chunks) -> Tuple[int, int, int, int, int, int]:
    """Type, shape and limit checks of ``attn_decode_extend``: ``(B, m, H, dh, cap, n_chunks)``.  Touches no device."""
    who = "attn_decode_extend"
    _theta_required(who, (("q", q), ("k_new", k_new), ("v_new", v_new), ("lengths", lengths), ("k_cache", k_cache),
                          ("v_cache", v_cache), ("workspace", workspace)))
    _place_fp32(who, (("q", q), ("k_new", k_new), ("v_new", v_new), ("x", x), ("prosody", prosody), ("Wp", Wp),
                      ("bp", bp), ("wm", wm), ("bm", bm), ("k_cache", k_cache), ("v_cache", v_cache),
                      ("workspace", workspace)), "the decode extend runs")
    if not isinstance(lengths, torch.Tensor):
        raise TypeError(f"{who}: lengths must be a torch.Tensor, got {type(lengths)}")
    if lengths.dtype != torch.int32:
        raise TypeError(f"{who}: lengths is {lengths.dtype}; the kernel reads and advances int32 lengths")
    if not lengths.is_contiguous():
        raise ValueError(f"{who}: lengths must be contiguous")
    if k_cache.dim() != 4 or v_cache.shape != k_cache.shape:
        raise ValueError(f"{who}: k_cache and v_cache are [B, H, cap, dh]; got {tuple(k_cache.shape)}, "
                         f"{tuple(v_cache.shape)}")
    B, H, cap, dh = k_cache.shape
    D = H * dh
    if H < 1 or dh % 4 != 0 or not 4 <= dh <= DECODE_MAX_HEAD:
        raise ValueError(f"{who}: dh={dh} must be a multiple of 4 in [4, {DECODE_MAX_HEAD}] (H={H})")
    if D > DECODE_MAX_D:
        raise ValueError(f"{who}: D = H dh = {D} exceeds {DECODE_MAX_D}")
    if not 1 <= cap <= DECODE_MAX_CAP:
        raise ValueError(f"{who}: cap={cap} must be in [1, {DECODE_MAX_CAP}]")
    if q.dim() != 3 or q.shape[0] != B or q.shape[2] != D:
        raise ValueError(f"{who}: q is [B, m, D] = ({B}, m, {D}), got {tuple(q.shape)}")
    m = q.shape[1]
    if not 1 <= m <= DECODE_EXTEND_MAX:
        raise ValueError(f"{who}: m={m} new tokens must be in [1, {DECODE_EXTEND_MAX}]")
    for n, t in (("k_new", k_new), ("v_new", v_new)):
        if tuple(t.shape) != (B, m, D):
            raise ValueError(f"{who}: {n} is [B, m, D] = ({B}, {m}, {D}), got {tuple(t.shape)}")
    if tuple(lengths.shape) != (B,):
        raise ValueError(f"{who}: lengths is [B] = ({B},), got {tuple(lengths.shape)}")
    if prosody is not None:
        if tuple(prosody.shape) != (B, m, 4):
            raise ValueError(f"{who}: prosody is [B, m, 4] = ({B}, {m}, 4), got {tuple(prosody.shape)}")
        _theta_required(who, (("Wp (with prosody)", Wp), ("bp (with prosody)", bp)))
        if tuple(Wp.shape) != (H, 4) or tuple(bp.shape) != (H,):
            raise ValueError(f"{who}: Wp is [H, 4] and bp [H] with H={H}; got {tuple(Wp.shape)}, {tuple(bp.shape)}")
    if (wm is None) != (bm is None):
        raise ValueError(f"{who}: wm and bm are the memory gate's weight and bias: give both or neither")
    if wm is not None:
        _theta_required(who, (("x (with wm)", x),))
        if wm.numel() != D or bm.numel() != 1:
            raise ValueError(f"{who}: wm holds D={D} weights and bm one bias; got {tuple(wm.shape)}, {tuple(bm.shape)}")
        if tuple(x.shape) != (B, m, D):
            raise ValueError(f"{who}: x is [B, m, D] = ({B}, {m}, {D}), got {tuple(x.shape)}")
    if n_chunks is None:
        n_chunks = attn_decode_chunks(cap)
    if isinstance(n_chunks, bool) or not isinstance(n_chunks, int):
        raise TypeError(f"{who}: n_chunks must be an int, got {type(n_chunks)}")
    if n_chunks < 1 or n_chunks * DECODE_CHUNK > cap + DECODE_CHUNK - 1:
        raise ValueError(f"{who}: n_chunks={n_chunks} must be in [1, ceil(cap / {DECODE_CHUNK})] with cap={cap}")
    if B * m * H * n_chunks > 0x7fffffff:
        raise ValueError(f"{who}: B m H n_chunks = {B * m * H * n_chunks} partials exceed 2^31 - 1")
    need = attn_decode_extend_workspace_floats(B, m, H, dh, n_chunks)
    if workspace.numel() < need:
        raise ValueError(f"{who}: workspace holds {workspace.numel()} floats, an extend of {m} needs {need}")
    return B, m, H, dh, cap, n_chunks


def _attn_decode_extend_counts(counts, lengths) -> None:
    """Type and shape checks of ``attn_decode_extend``'s ``counts``.  Touches no device; the values are never read."""
    who = "attn_decode_extend"
    if not isinstance(counts, torch.Tensor):
        raise TypeError(f"{who}: counts must be a torch.Tensor, got {type(counts)}")
    if counts.dtype != torch.int32:
        raise TypeError(f"{who}: counts is {counts.dtype}; the kernel reads int32 counts")
    if tuple(counts.shape) != tuple(lengths.shape):
        raise ValueError(f"{who}: counts is [B] = {tuple(lengths.shape)}, got {tuple(counts.shape)}")
    if not counts.is_contiguous():
        raise ValueError(f"{who}: counts must be contiguous")
    if counts.device != lengths.device:
        raise ValueError(f"{who}: counts is on {counts.device}, the other tensors on {lengths.device}")


def attn_decode_extend(q, k_new, v_new, x, prosody, Wp, bp, wm, bm, lengths, k_cache, v_cache, workspace,
                       n_chunks: Optional[int] = None, advance: bool = True, return_scale: bool = False,
                       counts: Optional[torch.Tensor] = None):
    """``m`` new tokens per row appended to a cache that holds a context, in two launches and one pass over K and V (the
    rule: ``include/aura_hip.h``, "Decode attention: extend"): ``q``, ``k_new``, ``v_new``, ``x`` [B, m, D] and
    ``prosody`` [B, m, 4] are ``attn_decode_step``'s arguments for ``m`` successive steps, ``1 <= m <=
    DECODE_EXTEND_MAX``.  Query ``j`` attends positions ``0 .. lengths[b] + j``; the ``m`` keys and values go to
    positions ``lengths[b] ..``.  Returns ``ctx`` [B, m, D].  A row with a negative length, or that does not fit whole
    (``lengths[b] + m > cap``), is inactive: zeros, nothing written.  ``advance`` adds ``m`` to the active rows'
    lengths.  ``workspace``: ``attn_decode_extend_workspace_floats`` fp32.  ``return_scale`` also returns ``s``
    [B, m, H].  Every bit of the results, the caches and the lengths is what the ``m`` steps leave.  No host sync.

    ``counts`` (int32 [B] on the tensors' device, never read on the host): row ``b`` takes only its first
    ``counts[b]`` of the ``m`` padded rows, which is what ``counts[b]`` steps leave; the rows from ``counts[b]`` on are
    read by nobody and their ``ctx`` and scales are zero.  A row fits by its own count (``lengths[b] + counts[b] <=
    cap``); a count outside ``[0, m]`` makes the row inactive, a count of 0 leaves it as it is.  ``advance`` adds
    ``counts[b]``.  ``None`` is the call without counts."""
    B, m, H, dh, cap, n_chunks = _attn_decode_extend_shapes(q, k_new, v_new, x, prosody, Wp, bp, wm, bm, lengths,
                                                            k_cache, v_cache, workspace, n_chunks)
    if counts is not None:
        _attn_decode_extend_counts(counts, lengths)
    if prosody is None:
        Wp = bp = None
    if wm is None:
        x = None
    dev = _theta_device("attn_decode_extend", (("q", q), ("k_new", k_new), ("v_new", v_new), ("x", x),
                                               ("prosody", prosody), ("Wp", Wp), ("bp", bp), ("wm", wm), ("bm", bm),
                                               ("lengths", lengths), ("k_cache", k_cache), ("v_cache", v_cache),
                                               ("workspace", workspace)),
                        wide=("q", "k_new", "v_new", "x", "wm", "k_cache", "v_cache", "workspace"))
    ctx = torch.empty(B, m, H * dh, dtype=torch.float32, device=dev)
    scale = torch.empty(B, m, H, dtype=torch.float32, device=dev) if return_scale else None
    if counts is not None:
        _need(counts, "attn_decode_extend: counts")
        check(lib().aura_attn_decode_extend_counts(_p(q), _p(k_new), _p(v_new), _p(x), _p(prosody), _p(Wp), _p(bp),
                                                   _p(wm), _p(bm), _p(lengths), _p(counts), _p(k_cache), _p(v_cache), B,
                                                   m, H, dh, cap, n_chunks, int(bool(advance)), _p(workspace),
                                                   workspace.numel() * 4, _p(ctx), _p(scale), _stream()),
              "aura_attn_decode_extend_counts")
        return (ctx, scale) if return_scale else ctx
    check(lib().aura_attn_decode_extend(_p(q), _p(k_new), _p(v_new), _p(x), _p(prosody), _p(Wp), _p(bp), _p(wm), _p(bm),
                                        _p(lengths), _p(k_cache), _p(v_cache), B, m, H, dh, cap, n_chunks,
                                        int(bool(advance)), _p(workspace), workspace.numel() * 4, _p(ctx), _p(scale),
                                        _stream()), "aura_attn_decode_extend")
    return (ctx, scale) if return_scale else ctx


# ---------------------------------------------------------------------------------------
# row linear (the rule: include/aura_hip.h, "Row linear")
# ---------------------------------------------------------------------------------------

ROW_LINEAR_MAX_ROWS = 32
ROW_LINEAR_MAX_K = 8192
ROW_LINEAR_ACTIVATIONS = (None, "gelu")
# the weight loads' cache policy: same bits either way; tools/fused_step_bench.py measures both
ROW_LINEAR_NONTEMPORAL = False


_RL_W, _RL_B, _RL_O = (tuple(f"{n}[{j}]" for j in range(3)) for n in ("weights", "biases", "out"))
_RL_PAD = ((), (None,), (None, None))


def _rl_f32(name: str, t) -> None:
    """One tensor of ``row_linear``: fp32 and contiguous.  (A decoding step makes four of these calls per layer and
    token on the host's clock, so the checks walk every tensor once and form no strings unless they raise.)"""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"row_linear: {name} must be a torch.Tensor, got {type(t)}")
    if t.dtype != torch.float32:
        raise TypeError(f"row_linear: {name} is {t.dtype}; the row linear kernel runs in fp32 only (fp32 is the limit: "
                        f"bf16 and fp16 are not supported)")
    if not t.is_contiguous():
        raise ValueError(f"row_linear: {name} must be contiguous")


def _row_linear_args(x, weights, biases, norm, eps, activation, residual, return_normed, out):
    """Type, shape and limit checks of ``row_linear``: ``(R, K, weights, biases, outs, gamma, beta, single)`` with
    the three tuples padded to three entries by ``None``.  Touches no device."""
    who = "row_linear"
    single = isinstance(weights, torch.Tensor)
    if single:
        weights = (weights,)
        biases = (biases,)
        out = None if out is None else (out,)
    if not isinstance(weights, (tuple, list)) or not 1 <= len(weights) <= 3:
        raise ValueError(f"{who}: weights is one tensor or a tuple of one to three, got "
                         f"{len(weights) if isinstance(weights, (tuple, list)) else type(weights)}")
    n = len(weights)
    if biases is None:
        biases = (None,) * n
    if isinstance(biases, torch.Tensor) or not isinstance(biases, (tuple, list)) or len(biases) != n:
        raise ValueError(f"{who}: biases come as the weights do: one entry (a tensor or None) per weight")
    if out is not None and (isinstance(out, torch.Tensor) or not isinstance(out, (tuple, list)) or len(out) != n):
        raise ValueError(f"{who}: out comes as the weights do: one tensor per weight")
    outs = (None,) * n if out is None else tuple(out)
    if x is None:
        raise ValueError(f"{who}: x is required")
    _rl_f32("x", x)
    if x.dim() != 2:
        raise ValueError(f"{who}: x is [R, K], got {tuple(x.shape)}")
    R, K = x.shape
    if not 1 <= R <= ROW_LINEAR_MAX_ROWS:
        raise ValueError(f"{who}: R={R} rows must be in [1, {ROW_LINEAR_MAX_ROWS}] (more rows are a library GEMM's work)")
    if K % 4 != 0 or not 4 <= K <= ROW_LINEAR_MAX_K:
        raise ValueError(f"{who}: K={K} must be a multiple of 4 in [4, {ROW_LINEAR_MAX_K}]")
    if activation is not None and activation != "gelu":
        raise ValueError(f"{who}: activation={activation!r}: None or 'gelu' (the exact, erf GELU)")
    total = 0
    for j in range(n):
        w, b, o = weights[j], biases[j], outs[j]
        if w is None:
            raise ValueError(f"{who}: {_RL_W[j]} is required")
        _rl_f32(_RL_W[j], w)
        if w.dim() != 2 or w.shape[1] != K or w.shape[0] < 1:
            raise ValueError(f"{who}: {_RL_W[j]} is [N, K] with K={K} and N >= 1 (nn.Linear's layout), got "
                             f"{tuple(w.shape)}")
        N = w.shape[0]
        total += N
        if b is not None:
            _rl_f32(_RL_B[j], b)
            if b.dim() != 1 or b.shape[0] != N:
                raise ValueError(f"{who}: {_RL_B[j]} is [N] = ({N},), got {tuple(b.shape)}")
        if o is not None:
            _rl_f32(_RL_O[j], o)
            if o.dim() != 2 or o.shape[0] != R or o.shape[1] != N:
                raise ValueError(f"{who}: {_RL_O[j]} is [R, N] = ({R}, {N}), got {tuple(o.shape)}")
    if total > 0x7fffffff:
        raise ValueError(f"{who}: the weights hold more than 2^31 - 1 output columns")
    gamma = beta = None
    if norm is not None:
        if not isinstance(norm, (tuple, list)) or len(norm) != 2 or norm[0] is None or norm[1] is None:
            raise ValueError(f"{who}: norm is (gamma, beta), the LayerNorm's weight and bias")
        gamma, beta = norm
        _rl_f32("gamma", gamma)
        _rl_f32("beta", beta)
        if K > DECODE_MAX_D:
            raise ValueError(f"{who}: the LayerNorm prologue holds a row in registers: K={K} exceeds {DECODE_MAX_D}")
        if gamma.dim() != 1 or beta.dim() != 1 or gamma.shape[0] != K or beta.shape[0] != K:
            raise ValueError(f"{who}: gamma and beta are [K] = ({K},); got {tuple(gamma.shape)}, {tuple(beta.shape)}")
        if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not eps >= 0.0:
            raise ValueError(f"{who}: eps={eps!r} must be a number that is not negative")
    elif return_normed:
        raise ValueError(f"{who}: return_normed needs norm=(gamma, beta)")
    if residual is not None:
        if n != 1:
            raise ValueError(f"{who}: a residual goes with a single weight matrix, not with {n}")
        _rl_f32("residual", residual)
        if residual.dim() != 2 or residual.shape[0] != R or residual.shape[1] != total:
            raise ValueError(f"{who}: residual is [R, N] = ({R}, {total}), got {tuple(residual.shape)}")
    pad = _RL_PAD[3 - n]
    return R, K, tuple(weights) + pad, tuple(biases) + pad, outs + pad, gamma, beta, single


def _rl_device(name: str, t, dev, wide: bool):
    """One tensor of ``row_linear`` on the one HIP device; the ``wide`` ones move as float4."""
    if not t.is_cuda:
        raise AuraDeviceError(f"row_linear: {name} is on {t.device}: aura_snn_rag_amd runs the hot path only as HIP "
                              f"kernels on an AMD GPU (no CPU/PyTorch fallback).")
    if dev is not None and t.device != dev:
        raise ValueError("row_linear: tensors are on different devices")
    if wide and t.data_ptr() % 16:
        raise ValueError(f"row_linear: {name} is not 16-byte aligned (a view into the middle of a buffer?)")
    return t.device


def row_linear(x, weights, biases=None, *, norm=None, eps: float = 1e-5, activation: Optional[str] = None,
               residual=None, return_normed: bool = False, out=None):
    """A linear layer for a handful of rows in one launch (the rule: ``include/aura_hip.h``, "Row linear"): ``x``
    [R, K] with R <= 32, ``weights`` one [N, K] tensor (``nn.Linear``'s layout) or a tuple of up to three that share
    ``x``, ``biases`` alike (entries may be ``None``).  ``norm=(gamma, beta)`` applies LayerNorm with ``eps`` to the rows
    first (K <= 2048); ``activation='gelu'`` is the exact GELU; ``residual`` [R, N] is added last (single weight only).
    Returns ``y`` [R, N], or a tuple of them for a tuple of weights; with ``return_normed`` ``(y, xh)``, ``xh`` [R, K] the
    normalised rows.  ``out`` (a tensor, or a tuple as the weights) receives the result.  fp32 only.  A row's bits are
    the same alone or in any batch, and the tuple form gives the bits of single calls.  No host sync."""
    R, K, W, b, outs, gamma, beta, single = _row_linear_args(x, weights, biases, norm, eps, activation, residual,
                                                              return_normed, out)
    dev = _rl_device("x", x, None, True)
    if gamma is not None:
        _rl_device("gamma", gamma, dev, True)
        _rl_device("beta", beta, dev, True)
    if residual is not None:
        _rl_device("residual", residual, dev, False)
    ys, N = [None, None, None], [0, 0, 0]
    for j in range(3):
        w = W[j]
        if w is None:
            break
        _rl_device(_RL_W[j], w, dev, True)
        if b[j] is not None:
            _rl_device(_RL_B[j], b[j], dev, False)
        N[j] = w.shape[0]
        if outs[j] is not None:
            _rl_device(_RL_O[j], outs[j], dev, False)
            ys[j] = outs[j]
        else:
            ys[j] = torch.empty((R, N[j]), dtype=torch.float32, device=dev)
    xh = torch.empty((R, K), dtype=torch.float32, device=dev) if return_normed else None
    check(lib().aura_row_linear(x.data_ptr(), R, K, _p(W[0]), _p(b[0]), _p(ys[0]), N[0], _p(W[1]), _p(b[1]), _p(ys[1]),
                                N[1], _p(W[2]), _p(b[2]), _p(ys[2]), N[2], _p(gamma), _p(beta), float(eps), _p(xh),
                                int(activation == "gelu"), _p(residual), int(ROW_LINEAR_NONTEMPORAL), _stream()),
          "aura_row_linear")
    y = ys[0] if single else tuple(t for t in ys if t is not None)
    return (y, xh) if return_normed else y


def _row_linear_gate_args(x, weight, bias, u, c, residual, out):
    """Type, shape and limit checks of ``row_linear_gate``: ``(R, K, N, ldw)``.  Touches no device."""
    who = "row_linear_gate"
    for name, t in (("x", x), ("weight", weight), ("u", u), ("c", c), ("residual", residual)):
        if t is None:
            raise ValueError(f"{who}: {name} is required")
    _rl_f32("x", x)
    if x.dim() != 2:
        raise ValueError(f"{who}: x is [R, K], got {tuple(x.shape)}")
    R, K = x.shape
    if not 1 <= R <= ROW_LINEAR_MAX_ROWS:
        raise ValueError(f"{who}: R={R} rows must be in [1, {ROW_LINEAR_MAX_ROWS}] (more rows are a library GEMM's work)")
    if K % 4 != 0 or not 4 <= K <= ROW_LINEAR_MAX_K:
        raise ValueError(f"{who}: K={K} must be a multiple of 4 in [4, {ROW_LINEAR_MAX_K}]")
    if not isinstance(weight, torch.Tensor):
        raise TypeError(f"{who}: weight must be a torch.Tensor, got {type(weight)}")
    if weight.dtype != torch.float32:
        raise TypeError(f"{who}: weight is {weight.dtype}; the row linear kernel runs in fp32 only")
    if weight.dim() != 2 or weight.shape[1] != K or weight.shape[0] < 1:
        raise ValueError(f"{who}: weight is [N, K] with K={K} and N >= 1 (nn.Linear's layout, or the left columns of a "
                         f"wider one), got {tuple(weight.shape)}")
    N = weight.shape[0]
    if N > 0x7fffffff:
        raise ValueError(f"{who}: the weight holds more than 2^31 - 1 output columns")
    if weight.stride(1) != 1:
        raise ValueError(f"{who}: a row of weight must be dense (stride 1), got {weight.stride(1)}")
    ldw = weight.stride(0) if N > 1 else max(K, weight.stride(0))
    if ldw < K or ldw % 4 != 0:
        raise ValueError(f"{who}: the rows of weight are {ldw} floats apart: the stride must be a multiple of 4 that is "
                         f"at least K={K}")
    if bias is not None:
        _rl_f32("bias", bias)
        if bias.dim() != 1 or bias.shape[0] != N:
            raise ValueError(f"{who}: bias is [N] = ({N},), got {tuple(bias.shape)}")
    for name, t in (("u", u), ("c", c), ("residual", residual), ("out", out)):
        if t is None:
            continue
        _rl_f32(name, t)
        if t.dim() != 2 or t.shape[0] != R or t.shape[1] != N:
            raise ValueError(f"{who}: {name} is [R, N] = ({R}, {N}), got {tuple(t.shape)}")
    return R, K, N, ldw


def row_linear_gate(x, weight, bias, u, c, residual, *, out=None):
    """The gated injection of a decoding step in one launch (the rule: ``include/aura_hip.h``, "Row linear: gate
    epilogue"): ``y = residual + sigmoid(x W^T + bias + u) * c`` with ``x`` [R, K], R <= 32, ``weight`` [N, K] whose rows
    may be further apart than K (``memory_gate[0].weight[:, :D]``: the view is read in place, nothing is copied), ``bias``
    [N] or ``None`` and the per-row ``u``, ``c``, ``residual`` [R, N].  Returns ``y`` [R, N] (``out`` receives it).  fp32
    only.  The dot product and a row's independence of its batch are ``row_linear``'s.  No host sync."""
    R, K, N, ldw = _row_linear_gate_args(x, weight, bias, u, c, residual, out)
    dev = _rl_device("x", x, None, True)
    _rl_device("weight", weight, dev, True)
    for name, t in (("bias", bias), ("u", u), ("c", c), ("residual", residual), ("out", out)):
        if t is not None:
            _rl_device(name, t, dev, False)
    y = out if out is not None else torch.empty((R, N), dtype=torch.float32, device=dev)
    check(lib().aura_row_linear_gate(x.data_ptr(), R, K, weight.data_ptr(), ldw, _p(bias), _p(u), _p(c), _p(residual),
                                     _p(y), N, int(ROW_LINEAR_NONTEMPORAL), _stream()),
          "aura_row_linear_gate")
    return y


def _row_linear_gif_args(x, weight, bias, T, decay, L, alpha, threshold, time_major, mix, out):
    """Type, shape and limit checks of ``row_linear_gif``: ``(R, K, N, out_shape, (res, m, gate))``.  Touches no
    device."""
    who = "row_linear_gif"
    if x is None or weight is None:
        raise ValueError(f"{who}: x and weight are required")
    _rl_f32("x", x)
    _rl_f32("weight", weight)
    if x.dim() != 2:
        raise ValueError(f"{who}: x is [R, K], got {tuple(x.shape)}")
    R, K = x.shape
    if not 1 <= R <= ROW_LINEAR_MAX_ROWS:
        raise ValueError(f"{who}: R={R} rows must be in [1, {ROW_LINEAR_MAX_ROWS}]")
    if K % 4 != 0 or not 4 <= K <= ROW_LINEAR_MAX_K:
        raise ValueError(f"{who}: K={K} must be a multiple of 4 in [4, {ROW_LINEAR_MAX_K}]")
    if weight.dim() != 2 or weight.shape[1] != K or weight.shape[0] < 1:
        raise ValueError(f"{who}: weight is [N, K] with K={K} and N >= 1, got {tuple(weight.shape)}")
    N = weight.shape[0]
    if bias is not None:
        _rl_f32("bias", bias)
        if bias.dim() != 1 or bias.shape[0] != N:
            raise ValueError(f"{who}: bias is [N] = ({N},), got {tuple(bias.shape)}")
    for name, v in (("T", T), ("L", L)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"{who}: {name} must be an int, got {type(v)}")
    if not 1 <= T <= ROW_LINEAR_MAX_ROWS:
        raise ValueError(f"{who}: T={T} must be in [1, {ROW_LINEAR_MAX_ROWS}]")
    if L < 1:
        raise ValueError(f"{who}: L={L} must be at least 1")
    for name, v in (("decay", decay), ("alpha", alpha), ("threshold", threshold)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise TypeError(f"{who}: {name} must be a number, got {type(v)}")
    if time_major and R % T != 0:
        raise ValueError(f"{who}: the time-major form takes whole tokens: R={R} is no multiple of T={T}")
    out_shape = (R // T, N) if time_major else (R, T, N)
    res = m = gate = None
    if mix is not None:
        if not time_major:
            raise ValueError(f"{who}: the mix goes with the time-major form (time_major=True)")
        if not isinstance(mix, (tuple, list)) or len(mix) != 3 or any(t is None for t in mix):
            raise ValueError(f"{who}: mix is (residual, m, gate): [tokens, N], [tokens, N] and one float")
        res, m, gate = mix
        for name, t in (("mix residual", res), ("mix m", m)):
            _rl_f32(name, t)
            if tuple(t.shape) != out_shape:
                raise ValueError(f"{who}: {name} is [tokens, N] = {out_shape}, got {tuple(t.shape)}")
        _rl_f32("mix gate", gate)
        if gate.numel() != 1:
            raise ValueError(f"{who}: mix gate is one float (the HybridFFN's gate parameter), got {tuple(gate.shape)}")
    if out is not None:
        _rl_f32("out", out)
        if tuple(out.shape) != out_shape:
            raise ValueError(f"{who}: out is {out_shape}, got {tuple(out.shape)}")
    return R, K, N, out_shape, (res, m, gate)


def row_linear_gif(x, weight, bias=None, *, T: int, decay: float, L: int, alpha: float, threshold: float,
                   time_major: bool = False, mix=None, out=None):
    """A skinny linear layer whose output feeds the GIF neuron loop in the same launch (the rule: ``include/aura_hip.h``,
    "Row linear: GIF epilogue"): ``x`` [R, K], R <= 32, ``weight`` [N, K], ``bias`` [N] or ``None``; every row or token
    starts from fresh neuron state.  ``time_major=False``: each row runs ``T`` steps on its own current -> spikes
    [R, T, N], the bits of ``gif_run(time_invariant=True)`` on ``row_linear``'s output.  ``time_major=True``: the rows are
    ``R / T`` tokens of ``T`` steps each -> the mean over T [R / T, N], the bits of ``gif_run(mean_out=True)``; with
    ``mix=(residual, m, gate)`` -> ``residual + ((1 - g) * m + g * mean)``, ``g = sigmoid(gate)`` read on the device.
    fp32 only, 1 <= T <= 32.  No host sync."""
    R, K, N, out_shape, (res, m, gate) = _row_linear_gif_args(x, weight, bias, T, decay, L, alpha, threshold,
                                                                time_major, mix, out)
    dev = _rl_device("x", x, None, True)
    _rl_device("weight", weight, dev, True)
    for name, t in (("bias", bias), ("mix residual", res), ("mix m", m), ("mix gate", gate), ("out", out)):
        if t is not None:
            _rl_device(name, t, dev, False)
    y = out if out is not None else torch.empty(out_shape, dtype=torch.float32, device=dev)
    check(lib().aura_row_linear_gif(x.data_ptr(), R, K, weight.data_ptr(), _p(bias), _p(y), N, int(T), float(decay),
                                    int(L), float(alpha), float(threshold), int(bool(time_major)), _p(res), _p(m),
                                    _p(gate), int(ROW_LINEAR_NONTEMPORAL), _stream()),
          "aura_row_linear_gif")
    return y


# ---------------------------------------------------------------------------------------
# memory attend (the rule: include/aura_hip.h, "Memory attend")
# ---------------------------------------------------------------------------------------

MEMORY_ATTEND_MAX_ROWS = 32
MEMORY_ATTEND_MAX_D = 2048
MEMORY_ATTEND_MAX_M = 32
MEMORY_ATTEND_MAX_HM = 1024


def _ma_f32(name: str, t, shape, what: str) -> None:
    """One tensor of ``memory_attend``: fp32, contiguous and of the given shape."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"memory_attend: {name} must be a torch.Tensor, got {type(t)}")
    if t.dtype != torch.float32:
        raise TypeError(f"memory_attend: {name} is {t.dtype}; the kernel runs in fp32 only (bf16 and fp16 tables are "
                        f"not supported)")
    if tuple(t.shape) != shape:
        raise ValueError(f"memory_attend: {name} is {what} = {shape}, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"memory_attend: {name} must be contiguous")


def _memory_attend_args(x, norm, G, s0, U, bias, eps, out):
    """Type, shape and limit checks of ``memory_attend``: ``(R, D, H, M, gamma, beta)``.  Touches no device."""
    who = "memory_attend"
    for name, t in (("x", x), ("G", G), ("s0", s0), ("U", U)):
        if t is None:
            raise ValueError(f"{who}: {name} is required")
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{who}: x must be a torch.Tensor, got {type(x)}")
    if x.dim() != 2:
        raise ValueError(f"{who}: x is [R, D], got {tuple(x.shape)}")
    R, D = x.shape
    _ma_f32("x", x, (R, D), "[R, D]")
    if not 1 <= R <= MEMORY_ATTEND_MAX_ROWS:
        raise ValueError(f"{who}: R={R} rows must be in [1, {MEMORY_ATTEND_MAX_ROWS}]")
    if D % 4 != 0 or not 4 <= D <= MEMORY_ATTEND_MAX_D:
        raise ValueError(f"{who}: D={D} must be a multiple of 4 in [4, {MEMORY_ATTEND_MAX_D}] (the row lives in "
                         f"registers)")
    if not isinstance(norm, (tuple, list)) or len(norm) != 2 or norm[0] is None or norm[1] is None:
        raise ValueError(f"{who}: norm is (gamma, beta), the LayerNorm's weight and bias")
    gamma, beta = norm
    _ma_f32("gamma", gamma, (D,), "[D]")
    _ma_f32("beta", beta, (D,), "[D]")
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not eps >= 0.0:
        raise ValueError(f"{who}: eps={eps!r} must be a number that is not negative")
    if not isinstance(G, torch.Tensor):
        raise TypeError(f"{who}: G must be a torch.Tensor, got {type(G)}")
    if G.dim() != 4 or G.shape[0] != R or G.shape[3] != D:
        raise ValueError(f"{who}: G is [R, H, M, D] = ({R}, H, M, {D}), got {tuple(G.shape)}")
    H, M = G.shape[1], G.shape[2]
    if not 1 <= M <= MEMORY_ATTEND_MAX_M:
        raise ValueError(f"{who}: M={M} memories must be in [1, {MEMORY_ATTEND_MAX_M}]")
    if not 1 <= H * M <= MEMORY_ATTEND_MAX_HM:
        raise ValueError(f"{who}: H M = {H} x {M} must be in [1, {MEMORY_ATTEND_MAX_HM}]")
    _ma_f32("G", G, (R, H, M, D), "[R, H, M, D]")
    _ma_f32("s0", s0, (R, H, M), "[R, H, M]")
    _ma_f32("U", U, (R, H, M, D), "[R, H, M, D]")
    if bias is not None:
        _ma_f32("bias", bias, (D,), "[D]")
    if out is not None:
        _ma_f32("out", out, (R, D), "[R, D]")
    return R, D, H, M, gamma, beta


def memory_attend(x, norm, G, s0, U, bias=None, *, eps: float = 1e-5, out=None):
    """The cross-attention injection of a decoding step over folded memories in one launch (the rule:
    ``include/aura_hip.h``, "Memory attend"): ``y = x + bias + sum_h sum_m p[h, m] U[:, h, m]`` with ``p[h] =
    softmax_m(G[:, h, m] . LayerNorm(x) + s0[:, h, m])``.  ``x`` [R, D] with R <= 32, ``norm=(gamma, beta)`` the
    LayerNorm's weight and bias, ``G`` and ``U`` [R, H, M, D], ``s0`` [R, H, M] (``MemoryAugmentedLayer.fold_memory``
    builds the three), ``bias`` [D] or ``None``.  Returns ``y`` [R, D] (``out`` receives it; it may alias no input).  fp32
    only.  A row's bits are the same alone or in any batch.  No host sync."""
    R, D, H, M, gamma, beta = _memory_attend_args(x, norm, G, s0, U, bias, eps, out)
    dev = None
    for name, t in (("x", x), ("gamma", gamma), ("beta", beta), ("G", G), ("s0", s0), ("U", U), ("bias", bias),
                    ("out", out)):
        if t is None:
            continue
        if not t.is_cuda:
            raise AuraDeviceError(f"memory_attend: {name} is on {t.device}: aura_snn_rag_amd runs the hot path only as "
                                  f"HIP kernels on an AMD GPU (no CPU/PyTorch fallback).")
        if dev is not None and t.device != dev:
            raise ValueError("memory_attend: tensors are on different devices")
        if name != "s0" and t.data_ptr() % 16:
            raise ValueError(f"memory_attend: {name} is not 16-byte aligned (a view into the middle of a buffer?)")
        dev = t.device
    y = out if out is not None else torch.empty((R, D), dtype=torch.float32, device=dev)
    check(lib().aura_memory_attend(x.data_ptr(), R, D, gamma.data_ptr(), beta.data_ptr(), float(eps), G.data_ptr(),
                                   s0.data_ptr(), U.data_ptr(), H, M, _p(bias), _p(y), _stream()),
          "aura_memory_attend")
    return y


# ---------------------------------------------------------------------------------------
# MoE zone (the rule: include/aura_hip.h, "MoE zone")
# ---------------------------------------------------------------------------------------

MOE_MAX_N = 1 << 24
MOE_MAX_DM = 256
MOE_MAX_HH = 512
MOE_MAX_HR = 256
MOE_MAX_E = 64
MOE_MAX_K = 8
MOE_MAX_LAYERS = 4
MOE_MAX_L = 64
MOE_TILE = 32


def _moe_f32(who: str, name: str, t, shape=None) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{who}: {name} must be a torch.Tensor, got {type(t)}")
    if t.dtype != torch.float32:
        raise TypeError(f"{who}: {name} is {t.dtype}; the MoE kernels run in fp32 only")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{who}: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be contiguous")


def _moe_x(who: str, x) -> Tuple[int, int]:
    _moe_f32(who, "x", x)
    if x.dim() != 2:
        raise ValueError(f"{who}: x is [N, Dm], got {tuple(x.shape)}")
    N, Dm = x.shape
    if N > MOE_MAX_N:
        raise ValueError(f"{who}: N={N} rows exceed {MOE_MAX_N}")
    if Dm % 4 or not 4 <= Dm <= MOE_MAX_DM:
        raise ValueError(f"{who}: Dm={Dm} must be a multiple of 4 in [4, {MOE_MAX_DM}]")
    return N, Dm


def _moe_device(who: str, named) -> torch.device:
    dev = None
    for name, t in named:
        if t is None:
            continue
        if not t.is_cuda:
            raise AuraDeviceError(f"{who}: {name} is on {t.device}: aura_snn_rag_amd runs the hot path only as HIP "
                                  f"kernels on an AMD GPU (no CPU/PyTorch fallback).")
        if dev is not None and t.device != dev:
            raise ValueError(f"{who}: tensors are on different devices")
        dev = t.device
    return dev


def moe_workspace_bytes(N: int, E: int, k: int) -> int:
    """Bytes of the plan ``moe_route`` leaves for ``moe_experts`` (host arithmetic, the C entry point's own layout)."""
    a256 = lambda n: (n + 255) // 256 * 256
    G = (N + MOE_TILE - 1) // MOE_TILE
    tiles = (N * k + MOE_TILE - 1) // MOE_TILE + E
    return 2 * a256(G * E * 4) + a256((E + 1) * 4) + a256(tiles * 12) + a256(N * k * 4)


def _moe_route_args(x, U, bU, bW, gate_w, gate_b, dt, k, temperature, attn_gain):
    """Type, shape and limit checks of ``moe_route``: ``(N, Dm, Hr, E, k)``.  Touches no device."""
    who = "moe_route"
    N, Dm = _moe_x(who, x)
    _moe_f32(who, "U", U)
    if U.dim() != 2 or U.shape[1] != Dm:
        raise ValueError(f"{who}: U is [Hr, Dm={Dm}], got {tuple(U.shape)}")
    Hr = U.shape[0]
    if not 1 <= Hr <= MOE_MAX_HR:
        raise ValueError(f"{who}: Hr={Hr} must be in [1, {MOE_MAX_HR}]")
    _moe_f32(who, "bU", bU, (Hr,))
    _moe_f32(who, "bW", bW, (Hr,))
    _moe_f32(who, "gate_w", gate_w)
    if gate_w.dim() != 2 or gate_w.shape[1] != Hr:
        raise ValueError(f"{who}: gate_w is [E, Hr={Hr}], got {tuple(gate_w.shape)}")
    E = gate_w.shape[0]
    if not 1 <= E <= MOE_MAX_E:
        raise ValueError(f"{who}: E={E} experts must be in [1, {MOE_MAX_E}]")
    _moe_f32(who, "gate_b", gate_b, (E,))
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= min(E, MOE_MAX_K):
        raise ValueError(f"{who}: k={k!r} must be an integer in [1, min(E, {MOE_MAX_K})] (pass min(top_k, E))")
    for name, v in (("dt", dt), ("temperature", temperature)):
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise TypeError(f"{who}: {name}={v!r} must be a number")
    if attn_gain is not None:
        _moe_f32(who, "attn_gain", attn_gain, (N,))
    return N, Dm, Hr, E, k


class MoeRouting:
    """What ``moe_route`` leaves: ``indices`` int32 [N, k], ``weights`` [N, k], ``probs`` [N, E] and ``plan``, the
    device-side grouping of the (token, slot) pairs by expert that ``moe_experts`` reads (a byte tensor; opaque)."""
    __slots__ = ("indices", "weights", "probs", "plan", "E", "k")

    def __init__(self, indices, weights, probs, plan, E, k):
        self.indices, self.weights, self.probs, self.plan, self.E, self.k = indices, weights, probs, plan, E, k


def moe_route(x, U, bU, bW, gate_w, gate_b, *, dt: float, k: int, temperature: float = 1.0, attn_gain=None) -> MoeRouting:
    """The liquid router in one launch and the plan of the expert launch in two more (the rule: ``include/aura_hip.h``,
    "MoE zone"): ``x`` [N, Dm]; ``U`` [Hr, Dm], ``bU``, ``bW`` [Hr] the cell's ``U.weight``, ``U.bias`` and ``W.bias``;
    ``gate_w`` [E, Hr], ``gate_b`` [E]; ``k = min(top_k, E)``; ``attn_gain`` [N] or ``None``.  fp32.  No host sync."""
    N, Dm, Hr, E, k = _moe_route_args(x, U, bU, bW, gate_w, gate_b, dt, k, temperature, attn_gain)
    dev = _moe_device("moe_route", (("x", x), ("U", U), ("bU", bU), ("bW", bW), ("gate_w", gate_w), ("gate_b", gate_b),
                                    ("attn_gain", attn_gain)))
    for name, t in (("x", x), ("U", U)):
        if t.data_ptr() % 16:
            raise ValueError(f"moe_route: {name} is not 16-byte aligned (a view into the middle of a buffer?)")
    indices = torch.empty((N, k), dtype=torch.int32, device=dev)
    weights = torch.empty((N, k), dtype=torch.float32, device=dev)
    probs = torch.empty((N, E), dtype=torch.float32, device=dev)
    nbytes = moe_workspace_bytes(N, E, k)
    plan = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    check(lib().aura_moe_route(x.data_ptr(), N, Dm, U.data_ptr(), bU.data_ptr(), bW.data_ptr(), Hr, float(dt),
                               gate_w.data_ptr(), gate_b.data_ptr(), E, k, float(temperature), _p(attn_gain),
                               indices.data_ptr(), weights.data_ptr(), probs.data_ptr(), plan.data_ptr(), nbytes,
                               _stream()), "aura_moe_route")
    return MoeRouting(indices, weights, probs, plan, E, k)


def _moe_expert_params(experts, gif):
    """Checks of ``moe_expert_table``: ``(E, layers, Dm, Hh)``.  ``experts[e]`` is the flat list ``[W_s, b_s, W_g, b_g] *
    layers + [W_r, b_r]`` of expert ``e``, ``gif[e][l] = (decay, L, alpha, threshold)``.  Touches no device."""
    who = "moe_expert_table"
    E = len(experts)
    if not 1 <= E <= MOE_MAX_E or len(gif) != E:
        raise ValueError(f"{who}: {E} experts (and {len(gif)} neuron settings) must be equal and in [1, {MOE_MAX_E}]")
    n = len(experts[0])
    if n < 6 or (n - 2) % 4:
        raise ValueError(f"{who}: an expert is 4 tensors per layer and 2 of the readout, got {n}")
    layers = (n - 2) // 4
    if layers > MOE_MAX_LAYERS:
        raise ValueError(f"{who}: num_layers={layers} exceeds {MOE_MAX_LAYERS}")
    _moe_f32(who, "experts[0] W_s", experts[0][0])
    if experts[0][0].dim() != 2:
        raise ValueError(f"{who}: a weight is a matrix, got {tuple(experts[0][0].shape)}")
    Hh, Dm = experts[0][0].shape
    if Dm % 4 or not 4 <= Dm <= MOE_MAX_DM:
        raise ValueError(f"{who}: Dm={Dm} must be a multiple of 4 in [4, {MOE_MAX_DM}]")
    if Hh % 4 or not 4 <= Hh <= MOE_MAX_HH:
        raise ValueError(f"{who}: Hh={Hh} must be a multiple of 4 in [4, {MOE_MAX_HH}]")
    for e, (ts, gs) in enumerate(zip(experts, gif)):
        if len(ts) != n or len(gs) != layers:
            raise ValueError(f"{who}: expert {e} has another number of layers")
        for l in range(layers):
            shapes = ((Hh, Dm if l == 0 else Hh), (Hh,), (Hh, Hh), (Hh,))
            for j, shp in enumerate(shapes):
                if ts[4 * l + j] is None:
                    raise ValueError(f"{who}: expert {e} layer {l}: a bias is required (bias=False is not supported)")
                _moe_f32(who, f"expert {e} layer {l} tensor {j}", ts[4 * l + j], shp)
            decay, L, alpha, thr = gs[l]
            if not 1 <= int(L) <= MOE_MAX_L or int(L) != L:
                raise ValueError(f"{who}: expert {e} layer {l}: L={L} must be an integer in [1, {MOE_MAX_L}]")
        _moe_f32(who, f"expert {e} readout.weight", ts[-2], (Dm, Hh))
        _moe_f32(who, f"expert {e} readout.bias", ts[-1], (Dm,))
    return E, layers, Dm, Hh


class MoeExpertTable:
    """The device table of per-expert parameter pointers and neuron settings ``moe_experts`` reads.  It holds the
    tensors it points to; nothing is copied or concatenated."""
    __slots__ = ("ptrs", "gif", "E", "layers", "Dm", "Hh", "held")

    def __init__(self, ptrs, gif, E, layers, Dm, Hh, held):
        self.ptrs, self.gif, self.E, self.layers, self.Dm, self.Hh, self.held = ptrs, gif, E, layers, Dm, Hh, held


def moe_expert_table(experts, gif) -> MoeExpertTable:
    """Build the pointer table of ``moe_experts`` (one small host-to-device copy; build it once and keep it while the
    parameters' storages stay).  See ``_moe_expert_params`` for the arguments."""
    E, layers, Dm, Hh = _moe_expert_params(experts, gif)
    flat = [t for ts in experts for t in ts]
    dev = _moe_device("moe_expert_table", ((f"tensor {i}", t) for i, t in enumerate(flat)))
    for i, t in enumerate(flat):
        if t.data_ptr() % 16:
            raise ValueError(f"moe_expert_table: tensor {i} is not 16-byte aligned")
    ptrs = torch.tensor([t.data_ptr() for t in flat], dtype=torch.int64).reshape(E, 4 * layers + 2).to(dev)
    g = torch.tensor([[[float(v) for v in gl] for gl in gs] for gs in gif], dtype=torch.float32).reshape(E, layers, 4)
    return MoeExpertTable(ptrs, g.to(dev), E, layers, Dm, Hh, flat)


def _moe_experts_args(x, routing, table, out, return_trace):
    """Checks of ``moe_experts``: ``(N, Dm, P)``.  Touches no device."""
    who = "moe_experts"
    N, Dm = _moe_x(who, x)
    if not isinstance(routing, MoeRouting):
        raise TypeError(f"{who}: routing is what moe_route returned, got {type(routing)}")
    if not isinstance(table, MoeExpertTable):
        raise TypeError(f"{who}: table is what moe_expert_table returned, got {type(table)}")
    if table.Dm != Dm:
        raise ValueError(f"{who}: the experts take Dm={table.Dm}, x has {Dm}")
    if table.E != routing.E:
        raise ValueError(f"{who}: routed over {routing.E} experts, the table holds {table.E}")
    if tuple(routing.indices.shape) != (N, routing.k):
        raise ValueError(f"{who}: the routing is of {routing.indices.shape[0]} rows, x has {N}")
    if out is not None:
        _moe_f32(who, "out", out, (N, Dm))
    return N, Dm, N * routing.k


def moe_experts(x, routing: MoeRouting, table: MoeExpertTable, *, out=None, return_trace: bool = False):
    """Every selected expert's ``SNNExpert.predict`` on its own tokens and the weighted sum, in two launches (the rule:
    ``include/aura_hip.h``, "MoE zone").  ``x`` is the tensor ``moe_route`` was given.  Returns ``(out [N, Dm], y [N, k,
    Dm], trace)``: ``y`` every pair's expert output, ``trace`` [N, k, layers, Hh] every layer's spikes or ``None``."""
    N, Dm, P = _moe_experts_args(x, routing, table, out, return_trace)
    dev = _moe_device("moe_experts", (("x", x), ("indices", routing.indices), ("table", table.ptrs), ("out", out)))
    if x.data_ptr() % 16 or (out is not None and out.data_ptr() % 16):
        raise ValueError("moe_experts: x or out is not 16-byte aligned")
    k = routing.k
    y = torch.empty((N, k, Dm), dtype=torch.float32, device=dev)
    res = out if out is not None else torch.empty((N, Dm), dtype=torch.float32, device=dev)
    trace = torch.empty((N, k, table.layers, table.Hh), dtype=torch.float32, device=dev) if return_trace else None
    check(lib().aura_moe_experts(x.data_ptr(), N, Dm, table.Hh, table.layers, table.E, k, table.ptrs.data_ptr(),
                                 table.gif.data_ptr(), routing.indices.data_ptr(), routing.weights.data_ptr(),
                                 y.data_ptr(), res.data_ptr(), _p(trace), routing.plan.data_ptr(),
                                 routing.plan.numel(), _stream()), "aura_moe_experts")
    return res, y, trace


def moe_forward(x, U, bU, bW, gate_w, gate_b, table: MoeExpertTable, *, dt: float, k: int, temperature: float = 1.0,
                attn_gain=None, out=None, return_trace: bool = False):
    """``moe_route`` then ``moe_experts``: five launches, no host sync.  Returns ``(out, routing, y, trace)``."""
    routing = moe_route(x, U, bU, bW, gate_w, gate_b, dt=dt, k=k, temperature=temperature, attn_gain=attn_gain)
    res, y, trace = moe_experts(x, routing, table, out=out, return_trace=return_trace)
    return res, routing, y, trace


# ---------------------------------------------------------------------------------------
# Poisson bridge (the rule: include/aura_hip.h, "Poisson bridge")
# ---------------------------------------------------------------------------------------

BRIDGE_MAX_N, BRIDGE_MAX_K, BRIDGE_MAX_H, BRIDGE_MAX_T = 1 << 24, MOE_MAX_DM, 4096, 64


def _bridge_f32(name: str, t, shape=None) -> None:
    who = "poisson_rate"
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{who}: {name} must be a torch.Tensor, got {type(t)}")
    if t.dtype != torch.float32:
        raise TypeError(f"{who}: {name} is {t.dtype}; the Poisson bridge runs in fp32 only (bf16 is not supported)")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{who}: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be contiguous")


def _poisson_rate_args(x, weight, bias, T, seed, streams, rows_per_stream, start, return_probs, return_spikes, out):
    """Type, shape and limit checks of ``poisson_rate``: ``(N, K, H, T, seed, B, S, start)`` with ``start`` the host's
    int (0 beside a device ``start``).  Touches no device and loads nothing."""
    who = "poisson_rate"
    _bridge_f32("x", x)
    if x.dim() != 2:
        raise ValueError(f"{who}: x is [N, K], got {tuple(x.shape)}")
    N, K = x.shape
    if N > BRIDGE_MAX_N:
        raise ValueError(f"{who}: N={N} rows exceed {BRIDGE_MAX_N}")
    if K % 4 or not 4 <= K <= BRIDGE_MAX_K:
        raise ValueError(f"{who}: K={K} must be a multiple of 4 in [4, {BRIDGE_MAX_K}]")
    _bridge_f32("weight", weight)
    if weight.dim() != 2 or weight.shape[1] != K:
        raise ValueError(f"{who}: weight is [H, K={K}] (nn.Linear's layout), got {tuple(weight.shape)}")
    H = weight.shape[0]
    if not 1 <= H <= BRIDGE_MAX_H:
        raise ValueError(f"{who}: H={H} channels must be in [1, {BRIDGE_MAX_H}]")
    if bias is not None:
        _bridge_f32("bias", bias, (H,))
    T = _sample_int(who, "T", T, 1, BRIDGE_MAX_T + 1)
    seed = _sample_int(who, "seed", seed, 0, 1 << 64)
    if (streams is None) != (rows_per_stream is None):
        raise ValueError(f"{who}: streams and rows_per_stream come together (default: every row its own stream, the "
                         f"row number)")
    if streams is None:
        B, S = N, 1
    else:
        S = _sample_int(who, "rows_per_stream", rows_per_stream, 1, max(N, 1) + 1)
        if N % S:
            raise ValueError(f"{who}: N={N} rows are not a multiple of rows_per_stream={S}")
        B = N // S
        if isinstance(streams, torch.Tensor):
            if streams.dtype not in (torch.int32, torch.int64) or tuple(streams.shape) != (B,) \
                    or not streams.is_contiguous():
                raise ValueError(f"{who}: streams is a contiguous int32 (the bits of a uint32) or int64 [B] = ({B},), "
                                 f"got {streams.dtype} {tuple(streams.shape)}")
        else:
            ids = np.asarray(streams)
            if ids.dtype.kind not in "iu" or ids.shape != (B,) or (ids.astype(np.int64) < 0).any() \
                    or (ids.astype(np.int64) >= (1 << 32)).any():
                raise ValueError(f"{who}: streams is [B] = ({B},) integers in [0, 2^32), got {streams!r}")
    if isinstance(start, torch.Tensor):
        if start.dtype != torch.int32 or tuple(start.shape) != (B,) or not start.is_contiguous():
            raise ValueError(f"{who}: a device start is a contiguous int32 [B] = ({B},), got {start.dtype} "
                             f"{tuple(start.shape)}")
        start0 = 0
    else:
        start0 = _sample_int(who, "start", start, 0, (1 << 31) - S + 1)
    if out is not None:
        _bridge_f32("out", out, (N, H))
    for name, t in (("x", x), ("weight", weight)):
        if t.data_ptr() % 16:
            raise ValueError(f"{who}: {name} is not 16-byte aligned (a view into the middle of a buffer?)")
    return N, K, H, T, seed, B, S, start0


def poisson_rate(x, weight, bias=None, *, T: int, seed: int, streams=None, rows_per_stream: Optional[int] = None,
                 start=0, return_probs: bool = False, return_spikes: bool = False, out=None):
    """``ContinuousToSpikeBridge`` ('poisson') and the mean over its timesteps in one launch (the rule:
    ``include/aura_hip.h``, "Poisson bridge"): ``x`` [N, K], ``weight`` [H, K], ``bias`` [H] or ``None`` ->
    ``rate`` [N, H], the mean over ``T`` steps of ``spike = u < sigmoid(x W^T + b)``.  The uniforms are Philox4x32-10 under
    ``seed``, keyed by (channel, timestep group, position, stream): row ``n = b S + i`` of stream ``streams[b]`` (int32
    holding the bits of a uint32, int64 taken modulo 2^32, or ints in [0, 2^32)) stands at position ``start[b] + i``,
    ``S = rows_per_stream``; ``start`` is an int or an int32 [B] device tensor the host never reads.  Default: row ``n``
    is stream ``n``, one row each.  A row's bits depend only on its own ``x`` row, stream, position and seed.

    Returns ``rate``, written into ``out`` [N, H] if given; with ``return_probs`` and / or ``return_spikes`` a tuple
    ``(rate, probs [N, H], spikes [N, T, H])`` of those asked for, in this order.  fp32 only.  No host sync."""
    N, K, H, T, seed, B, S, start0 = _poisson_rate_args(x, weight, bias, T, seed, streams, rows_per_stream, start,
                                                       return_probs, return_spikes, out)
    who = "poisson_rate"
    dev = None
    for name, t in (("x", x), ("weight", weight), ("bias", bias), ("out", out), ("streams", streams), ("start", start)):
        if not isinstance(t, torch.Tensor):
            continue
        if not t.is_cuda:
            raise AuraDeviceError(f"{who}: {name} is on {t.device}: aura_snn_rag_amd runs the hot path only as HIP "
                                  f"kernels on an AMD GPU (no CPU/PyTorch fallback).")
        if dev is not None and t.device != dev:
            raise ValueError(f"{who}: tensors are on different devices")
        dev = t.device
    if streams is None:
        streams = torch.arange(N, dtype=torch.int32, device=dev)
    elif not isinstance(streams, torch.Tensor):
        streams = torch.as_tensor(np.asarray(streams, dtype=np.int64).astype(np.uint32).view(np.int32), device=dev)
    elif streams.dtype == torch.int64:
        streams = streams.to(torch.int32)                           # modulo 2^32: the low word's bits
    rate = out if out is not None else torch.empty((N, H), dtype=torch.float32, device=dev)
    probs = torch.empty((N, H), dtype=torch.float32, device=dev) if return_probs else None
    spikes = torch.empty((N, T, H), dtype=torch.float32, device=dev) if return_spikes else None
    if N > 0:                                                       # (no rows: nothing to launch, nothing to point at)
        check(lib().aura_poisson_rate(x.data_ptr(), N, K, weight.data_ptr(), _p(bias), H, T, seed, streams.data_ptr(),
                                      S, start0, _p(start) if isinstance(start, torch.Tensor) else None,
                                      rate.data_ptr(), _p(probs), _p(spikes), _stream()), "aura_poisson_rate")
    if not (return_probs or return_spikes):
        return rate
    return (rate,) + tuple(t for t in (probs, spikes) if t is not None)


# ---------------------------------------------------------------------------------------
# next token (the rule: include/aura_hip.h, "Next token")
# ---------------------------------------------------------------------------------------

SAMPLE_MAX_K, SAMPLE_MAX_V = 1024, 131072
PENALTY_RULES = {"divide": 0, "signed": 1}


def _sample_int(who: str, name: str, v, lo: int, hi: int) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise TypeError(f"{who}: {name} must be an int, got {type(v)}")
    if not lo <= int(v) < hi:
        raise ValueError(f"{who}: {name}={v} must be in [{lo}, {hi})")
    return int(v)


def _sample_args(logits, seen, finished, stream_ids, penalty, penalty_rule, temperature, top_k, top_p, seed, step,
                 eos_id, pad_id, out):
    """Type, shape and limit checks of ``sample_next``: ``(B, V, row_stride, scalars)`` with ``scalars`` the library's
    arguments from ``penalty`` to ``pad_id``.  Touches no device and loads nothing."""
    who = "sample_next"
    if not isinstance(logits, torch.Tensor):
        raise TypeError(f"{who}: logits must be a torch.Tensor, got {type(logits)}")
    if logits.dtype != torch.float32:
        raise TypeError(f"{who}: logits is {logits.dtype}; the sampler reads fp32 logits only (bf16 and fp16 are not "
                        f"supported)")
    if logits.dim() != 2:
        raise ValueError(f"{who}: logits is [B, V], got {tuple(logits.shape)}")
    B, V = logits.shape
    if B < 1 or not 1 <= V <= SAMPLE_MAX_V:
        raise ValueError(f"{who}: logits is [B, V] with B >= 1 and 1 <= V <= {SAMPLE_MAX_V}, got {tuple(logits.shape)}")
    if V > 1 and logits.stride(1) != 1:
        raise ValueError(f"{who}: the vocabulary axis of logits must be dense (stride 1), got {logits.stride(1)}")
    row_stride = logits.stride(0) if B > 1 else V
    if row_stride < V:
        raise ValueError(f"{who}: the rows of logits overlap (row stride {row_stride} < V = {V})")
    for n, t, shape in (("seen", seen, (B, V)), ("finished", finished, (B,))):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{who}: {n} must be a torch.Tensor, got {type(t)}")
        if t.dtype != torch.uint8:
            raise TypeError(f"{who}: {n} is {t.dtype}; the row state is uint8")
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{who}: {n} is a contiguous {list(shape)}, got {tuple(t.shape)}")
    if stream_ids is not None:
        if not isinstance(stream_ids, torch.Tensor):
            ids = np.asarray(stream_ids)
            if ids.dtype.kind not in "iu" or ids.shape != (B,) or (ids.astype(np.int64) < 0).any() \
                    or (ids.astype(np.int64) >= (1 << 32)).any():
                raise ValueError(f"{who}: stream_ids is [B] = ({B},) integers in [0, 2^32), got {stream_ids!r}")
        elif stream_ids.dtype != torch.int64 or tuple(stream_ids.shape) != (B,) or not stream_ids.is_contiguous():
            raise ValueError(f"{who}: stream_ids is a contiguous int64 [B] = ({B},), got {stream_ids.dtype} "
                             f"{tuple(stream_ids.shape)}")
    if out is not None:
        if not isinstance(out, torch.Tensor):
            raise TypeError(f"{who}: out must be a torch.Tensor, got {type(out)}")
        if out.dtype != torch.int64:
            raise TypeError(f"{who}: out is {out.dtype}; tokens are int64")
        if tuple(out.shape) != (B,) or (B > 1 and out.stride(0) < 1):
            raise ValueError(f"{who}: out is [B] = ({B},) with a positive stride (a column of the generated buffer), got "
                             f"{tuple(out.shape)} stride {out.stride()}")
    if penalty_rule not in PENALTY_RULES:
        raise ValueError(f"{who}: penalty_rule must be 'divide' or 'signed', got {penalty_rule!r}")
    top_k = _sample_int(who, "top_k", top_k, 0, SAMPLE_MAX_K + 1)
    vals = {}
    for n, v in (("penalty", penalty), ("temperature", temperature), ("top_p", top_p)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise TypeError(f"{who}: {n} must be a number, got {type(v)}")
        with np.errstate(over="ignore"):
            vals[n] = float(np.float32(v))
    if not (np.isfinite(vals["temperature"]) and vals["temperature"] >= 0.0):
        raise ValueError(f"{who}: temperature={temperature} must be finite and not negative (0 is greedy)")
    if not (np.isfinite(vals["penalty"]) and vals["penalty"] > 0.0):
        raise ValueError(f"{who}: penalty={penalty} must be finite and positive")
    if not vals["top_p"] >= 0.0:
        raise ValueError(f"{who}: top_p={top_p} must be a number >= 0")
    if top_k == 0 and vals["top_p"] < 1.0:
        raise ValueError(f"{who}: top_p={top_p} < 1 needs 1 <= top_k <= {SAMPLE_MAX_K}: a nucleus over the whole "
                         f"vocabulary (top_k=0) is not built, the candidate set is capped at {SAMPLE_MAX_K}")
    seed = _sample_int(who, "seed", seed, 0, 1 << 64)
    step = _sample_int(who, "step", step, 0, 1 << 64)
    eos = -1 if eos_id is None else _sample_int(who, "eos_id", eos_id, 0, 1 << 62)
    pad = _sample_int(who, "pad_id", pad_id, -(1 << 62), 1 << 62)
    return B, V, row_stride, (vals["penalty"], PENALTY_RULES[penalty_rule], vals["temperature"], top_k, vals["top_p"],
                              seed, step, eos, pad)


def sample_next(logits, *, seen=None, finished=None, stream_ids=None, penalty: float = 1.0,
                penalty_rule: str = "divide", temperature: float = 1.0, top_k: int = 50, top_p: float = 0.9,
                seed: int = 0, step: int = 0, eos_id: Optional[int] = None, pad_id: int = 0, out=None,
                return_candidates: bool = False):
    """The next token of every row of fp32 ``logits`` [B, V] (rows may be a strided view: the output head's result is
    read as it is) in one launch -- the rule: ``include/aura_hip.h``, "Next token".  Repetition penalty over the tokens
    marked in ``seen`` (uint8 [B, V]; ``penalty_rule`` ``'divide'``: the reference ``generate``'s line, ``'signed'``: its
    ``apply_repetition_penalty``), ``temperature`` (0: greedy argmax, nothing drawn), exactly ``min(top_k, V)``
    candidates by (logit descending, id ascending), the nucleus ``top_p`` over them, and a Gumbel-max draw whose random
    numbers are a function of ``(seed, step, stream, token id)`` alone; ``stream_ids`` (int64 [B] or ints) default to the
    row numbers, so a row alone with its stream draws what it draws in the batch.  ``top_k=0`` samples the whole
    vocabulary and needs ``top_p >= 1``.  Row state on the device: a row with ``finished`` (uint8 [B]) set writes
    ``pad_id`` and nothing else; otherwise the token's byte of ``seen`` is set and, with ``eos_id``, ``finished`` where
    the token is ``eos_id``.  A row without a finite logit returns -1.

    Returns int64 [B], or writes into ``out`` (int64 [B], any positive stride: a column of a [B, T] buffer) and returns
    it.  ``return_candidates``: also a dict of the kernel's own decisions -- ``ids`` int32, ``z``, ``cum``, ``d`` fp32
    [B, k'] and ``n_kept`` int32 [B] (``top_k >= 1``), ``d`` [B, V] (``top_k=0``), empty for greedy; rows that entered
    finished keep the fill (-1 / -inf / 0).  No host sync."""
    B, V, row_stride, scalars = _sample_args(logits, seen, finished, stream_ids, penalty, penalty_rule, temperature,
                                             top_k, top_p, seed, step, eos_id, pad_id, out)
    who = "sample_next"
    for n, t in (("logits", logits), ("seen", seen), ("finished", finished), ("out", out),
                 ("stream_ids", stream_ids if isinstance(stream_ids, torch.Tensor) else None)):
        if t is not None and not t.is_cuda:
            raise AuraDeviceError(f"{who}: {n} is on {t.device}: the sampler runs only as a HIP kernel on an AMD GPU (no "
                                  f"CPU/PyTorch fallback).")
        if t is not None and t.device != logits.device:
            raise ValueError(f"{who}: tensors are on different devices")
    dev = logits.device
    if stream_ids is not None and not isinstance(stream_ids, torch.Tensor):
        stream_ids = torch.as_tensor(np.asarray(stream_ids, dtype=np.int64), device=dev)
    tokens = torch.empty(B, dtype=torch.int64, device=dev) if out is None else out
    temperature32, k_top = scalars[2], scalars[3]
    cand = {}
    if return_candidates and temperature32 != 0.0:
        ninf = float("-inf")
        if k_top == 0:
            cand = dict(d=torch.full((B, V), ninf, dtype=torch.float32, device=dev))
        else:
            k = min(k_top, V)
            cand = dict(ids=torch.full((B, k), -1, dtype=torch.int32, device=dev),
                        z=torch.full((B, k), ninf, dtype=torch.float32, device=dev),
                        cum=torch.full((B, k), ninf, dtype=torch.float32, device=dev),
                        d=torch.full((B, k), ninf, dtype=torch.float32, device=dev),
                        n_kept=torch.zeros(B, dtype=torch.int32, device=dev))
    L = lib()
    nbytes = L.aura_sample_workspace_bytes(B, V, k_top, temperature32)
    if nbytes < 0:
        raise ValueError(f"{who}: unsupported size")
    base = _workspace(dev, nbytes) if nbytes else None
    check(L.aura_sample_next(_p(logits), row_stride, B, V, _p(seen), _p(finished), _p(stream_ids), *scalars,
                             _p(tokens), tokens.stride(0) if B > 1 else 1, _p(cand.get("ids")), _p(cand.get("z")),
                             _p(cand.get("cum")), _p(cand.get("d")), _p(cand.get("n_kept")), base, nbytes, _stream()),
          "aura_sample_next")
    return (tokens, cand) if return_candidates else tokens


# ---------------------------------------------------------------------------------------
# surrogate-gradient training path + prosody-modulated GIF (fp32 and bf16)
# ---------------------------------------------------------------------------------------

def _same_dtype(dtype, shape, *named) -> None:
    for t, n in named:
        _need(t, n, dtype)
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{n}: expected shape {tuple(shape)}, got {tuple(t.shape)}")


def gif_train_forward(h, spikes, v, theta, save_a, save_theta, decay: float, L: int, alpha: float,
                      threshold: float) -> None:
    """h [rows, T, H] -> spikes, save_a, save_theta [rows, T, H]; v, theta [rows, H] in/out (fp32 or bf16)."""
    rows, T, H = h.shape
    dt, code = _fp32_or_bf16(h, None)
    _same_dtype(dt, (rows, T, H), (h, "h"), (spikes, "spikes"), (save_a, "save_a"), (save_theta, "save_theta"))
    _same_dtype(dt, (rows, H), (v, "v"), (theta, "theta"))
    check(lib().aura_gif_train_forward(_p(h), _p(spikes), _p(v), _p(theta), _p(save_a), _p(save_theta),
                                       decay, int(L), alpha, threshold, rows, T, H, code, _stream()),
          "aura_gif_train_forward")


def gif_backward(save_a, save_theta, g_spikes, g_h, g_v, g_theta, decay: float, L: int, alpha: float,
                 threshold: float) -> None:
    """g_v, g_theta [rows, H]: gradients of the final state in, of the initial state out (fp32 or bf16)."""
    rows, T, H = save_a.shape
    dt, code = _fp32_or_bf16(save_a, None)
    _same_dtype(dt, (rows, T, H), (save_a, "save_a"), (save_theta, "save_theta"), (g_spikes, "g_spikes"),
                (g_h, "g_h"))
    _same_dtype(dt, (rows, H), (g_v, "g_v"), (g_theta, "g_theta"))
    check(lib().aura_gif_backward(_p(save_a), _p(save_theta), _p(g_spikes), _p(g_h), _p(g_v), _p(g_theta),
                                  decay, int(L), alpha, threshold, rows, T, H, code, _stream()),
          "aura_gif_backward")


def lif_train_forward(x, mem_in, beta, threshold, spikes, mem_out, pre) -> None:
    """One recording LIF step, [B, size]; fp32 or all bf16."""
    B, size = x.shape
    dt, code = _fp32_or_bf16(x, "lif_train_forward")
    _same_dtype(dt, (B, size), (x, "x"), (mem_in, "mem_in"), (spikes, "spikes"), (mem_out, "mem_out"), (pre, "pre"))
    _same_dtype(dt, (size,), (beta, "beta"), (threshold, "threshold"))
    check(lib().aura_lif_train_forward(_p(x), _p(mem_in), _p(beta), _p(threshold), _p(spikes), _p(mem_out), _p(pre),
                                       B, size, code, _stream()), "aura_lif_train_forward")


def lif_backward(pre, g_spikes, g_mem, beta, threshold, slope, g_x, g_mem_prev, raw_slope) -> None:
    """raw_slope [B, size] is fp32 in both forms (sum it over the batch for d/d slope)."""
    B, size = pre.shape
    dt, code = _fp32_or_bf16(pre, "lif_backward")
    _same_dtype(dt, (B, size), (pre, "pre"), (g_spikes, "g_spikes"), (g_mem, "g_mem"), (g_x, "g_x"),
                (g_mem_prev, "g_mem_prev"))
    _same_dtype(torch.float32, (B, size), (raw_slope, "raw_slope"))
    _same_dtype(dt, (size,), (beta, "beta"), (threshold, "threshold"), (slope, "slope"))
    check(lib().aura_lif_backward(_p(pre), _p(g_spikes), _p(g_mem), _p(beta), _p(threshold), _p(slope), _p(g_x),
                                  _p(g_mem_prev), _p(raw_slope), B, size, code, _stream()), "aura_lif_backward")


def gif_prosody_run(h, gains, spikes, v, theta, decay: float, L: int, alpha: float, threshold: float,
                    strength: float) -> None:
    """h, spikes [rows, T, H]; gains [rows, T] or None; v, theta [rows, H] in/out.  fp32, or everything
    (gains included) bf16."""
    rows, T, H = h.shape
    dt, code = _fp32_or_bf16(h, "gif_prosody_run")
    _same_dtype(dt, (rows, T, H), (h, "h"), (spikes, "spikes"))
    _same_dtype(dt, (rows, H), (v, "v"), (theta, "theta"))
    if gains is not None:
        _same_dtype(dt, (rows, T), (gains, "gains"))
    check(lib().aura_gif_prosody_run(_p(h), _p(gains), _p(spikes), _p(v), _p(theta), decay, int(L), alpha, threshold,
                                     strength, rows, T, H, code, _stream()), "aura_gif_prosody_run")


def gif_prosody_train_forward(h, gains, spikes, v, theta, save_a, save_theta, decay: float, L: int, alpha: float,
                              threshold: float, strength: float) -> None:
    rows, T, H = h.shape
    dt, code = _fp32_or_bf16(h, "gif_prosody_train_forward")
    _same_dtype(dt, (rows, T, H), (h, "h"), (spikes, "spikes"), (save_a, "save_a"), (save_theta, "save_theta"))
    _same_dtype(dt, (rows, H), (v, "v"), (theta, "theta"))
    if gains is not None:
        _same_dtype(dt, (rows, T), (gains, "gains"))
    check(lib().aura_gif_prosody_train_forward(_p(h), _p(gains), _p(spikes), _p(v), _p(theta), _p(save_a),
                                               _p(save_theta), decay, int(L), alpha, threshold, strength, rows, T, H,
                                               code, _stream()), "aura_gif_prosody_train_forward")


def gif_prosody_backward(save_a, save_theta, h, gains, g_spikes, g_h, g_gains, g_v, g_theta, decay: float, L: int,
                         alpha: float, threshold: float, strength: float) -> None:
    """g_gains [rows, T], fp32 in both forms, must be zero on entry (channels are accumulated into it)."""
    rows, T, H = save_a.shape
    dt, code = _fp32_or_bf16(save_a, "gif_prosody_backward")
    _same_dtype(dt, (rows, T, H), (save_a, "save_a"), (save_theta, "save_theta"), (h, "h"), (g_spikes, "g_spikes"),
                (g_h, "g_h"))
    _same_dtype(dt, (rows, H), (g_v, "g_v"), (g_theta, "g_theta"))
    if gains is not None:
        _same_dtype(dt, (rows, T), (gains, "gains"))
        _same_dtype(torch.float32, (rows, T), (g_gains, "g_gains"))
    check(lib().aura_gif_prosody_backward(_p(save_a), _p(save_theta), _p(h), _p(gains), _p(g_spikes), _p(g_h),
                                          _p(g_gains), _p(g_v), _p(g_theta), decay, int(L), alpha, threshold, strength,
                                          rows, T, H, code, _stream()), "aura_gif_prosody_backward")


# ---------------------------------------------------------------------------------------
# episodic bank
# ---------------------------------------------------------------------------------------

def bank_row_norms(bank, inv_norm, row0: int, n: int) -> None:
    """inv_norm[r] = 1 / max(||bank[r]||, 1e-12) for r in [row0, row0 + n): a zero row gets 1 / 1e-12f, no inf."""
    _need(bank, "bank", torch.float32); _need(inv_norm, "inv_norm", torch.float32)
    M, D = bank.shape
    if row0 < 0 or n < 0 or row0 + n > M or inv_norm.numel() != M:
        raise ValueError("bank_row_norms: range out of bounds")
    check(lib().aura_bank_row_norms(_p(bank), _p(inv_norm), row0, n, D, _stream()),
          "aura_bank_row_norms")


def bank_shadow_update(bank, inv_norm, shadow, rho, row0: int = 0, n: Optional[int] = None, slots=None) -> None:
    """shadow[r] = bf16(bank[r] * inv_norm[r]) (the normalised row) and rho[r] = its L2 rounding
    residual, for the rows ``slots`` (int64 [n], device) or [row0, row0 + n)."""
    _need(bank, "bank", torch.float32); _need(shadow, "shadow", torch.bfloat16)
    _need(inv_norm, "inv_norm", torch.float32); _need(rho, "rho", torch.float32)
    M, D = bank.shape
    if shadow.shape != bank.shape or D % 8 or inv_norm.numel() != M or rho.numel() != M:
        raise ValueError("bank_shadow_update: shadow must match the bank, D % 8 == 0, inv_norm / rho [rows]")
    if slots is not None:
        _need(slots, "slots", torch.int64)
        n = slots.numel()
    elif n is None:
        n = M - row0
    if row0 < 0 or n < 0 or (slots is None and row0 + n > M):
        raise ValueError("bank_shadow_update: range out of bounds")
    check(lib().aura_bank_shadow_update(_p(bank), _p(inv_norm), _p(shadow), _p(rho), _p(slots), row0, n, D,
                                        _stream()), "aura_bank_shadow_update")


def make_shadow(bank, inv_norm, count: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(shadow bf16 [M, D], rho fp32 [M]) of rows [0, count) of a bank whose 1/||row|| are current."""
    M, D = bank.shape
    shadow = torch.empty(M, D, dtype=torch.bfloat16, device=bank.device)
    rho = torch.zeros(M, dtype=torch.float32, device=bank.device)
    bank_shadow_update(bank, inv_norm, shadow, rho, 0, M if count is None else count)
    return shadow, rho


def bank_write(bank, loc, meta, inv_norm, feats, slots, cur_loc, now: float,
               centroids=None, centroid_counts=None, eff_k: int = 0, distinct_slots: bool = False,
               serial: bool = False) -> None:
    """Write feats[n, D] into rows ``slots`` (int64 [n], device).  With ``centroids`` the reference's online
    nearest-centroid / running-mean update runs in row order (``hippocampal.py:218-230``): through
    ``aura_bank_write_online`` (distances out of the serial chain, same bits) when the caller vouches that the
    slots are distinct, else -- or with ``serial`` (tests: the checker) -- through the one-workgroup kernel."""
    for t, n_ in ((bank, "bank"), (loc, "loc"), (meta, "meta"), (inv_norm, "inv_norm"),
                  (feats, "feats"), (cur_loc, "cur_loc")):
        _need(t, n_, torch.float32)
    _need(slots, "slots", torch.int64)
    M, D = bank.shape
    n = feats.shape[0]
    sd = loc.shape[1]
    if feats.shape != (n, D) or slots.numel() != n or meta.shape != (M, 4) or \
            loc.shape[0] != M or cur_loc.numel() != sd or inv_norm.numel() != M:
        raise ValueError("bank_write: shape mismatch")
    # slots are planned on the host by HippocampalFormation._plan_slots (always within [0, M))
    if centroids is not None:
        _need(centroids, "centroids", torch.float32)
        _need(centroid_counts, "centroid_counts", torch.float32)
        if centroids.shape[1] != D or not (0 < eff_k <= centroids.shape[0] <= 256) or \
                centroid_counts.numel() < eff_k:
            raise ValueError("bank_write: centroid shape mismatch")
    if centroids is not None and distinct_slots and not serial and n > 0:
        L = lib()
        nbytes = L.aura_bank_write_online_workspace_bytes(n)
        base = _workspace(bank.device, nbytes)
        check(L.aura_bank_write_online(_p(bank), _p(loc), _p(meta), _p(inv_norm), _p(centroids),
                                       _p(centroid_counts), eff_k, _p(feats), _p(slots), _p(cur_loc), sd,
                                       now, n, D, base, nbytes, _stream()), "aura_bank_write_online")
        return
    check(lib().aura_bank_write(_p(bank), _p(loc), _p(meta), _p(inv_norm), _p(centroids),
                                _p(centroid_counts), eff_k, _p(feats), _p(slots), _p(cur_loc), sd,
                                now, n, D, _stream()), "aura_bank_write")


def bank_decay(meta, rate: float, count: int) -> None:
    _need(meta, "meta", torch.float32)
    if count < 0 or count > meta.shape[0] or meta.shape[1] != 4:
        raise ValueError("bank_decay: bad count")
    check(lib().aura_bank_decay(_p(meta), rate, count, _stream()), "aura_bank_decay")


# Scratch memory and the overflow flag are per (device, stream): two recalls in flight on different
# HIP streams never share candidate lists, thresholds or flags.  A buffer that has to grow is replaced
# (the old one is returned to torch's caching allocator, which keeps it alive for work already queued
# on its stream).
_workspaces = {}
_ovf_flags = {}


def _wkey(device):
    return (device, torch.cuda.current_stream(device).cuda_stream)


def _workspace(device, nbytes: int) -> int:
    """Base address (256-byte aligned) of this (device, stream)'s scratch of at least ``nbytes``."""
    key = _wkey(device)
    ws = _workspaces.get(key)
    if ws is None or ws[0] < nbytes:
        buf = torch.empty(nbytes + 256, dtype=torch.uint8, device=device)
        ws = _workspaces[key] = (nbytes, (buf.data_ptr() + 255) // 256 * 256, buf)   # (usable bytes, base, buffer)
    return ws[1]


def _overflow_flag(device) -> torch.Tensor:
    """int32 [1], reset by the library's prep kernel on every call."""
    key = _wkey(device)
    f = _ovf_flags.get(key)
    if f is None:
        f = _ovf_flags[key] = torch.zeros(1, dtype=torch.int32, device=device)
    return f


def _workspace_view(device, nbytes: int) -> torch.Tensor:
    """The first ``nbytes`` of this (device, stream)'s scratch as a uint8 tensor (what a kernel left there)."""
    base = _workspace(device, nbytes)
    buf = _workspaces[_wkey(device)][2]
    off = base - buf.data_ptr()
    return buf[off:off + nbytes]


def _check_meta(meta, count: int, who: str) -> None:
    _need(meta, "meta", torch.float32)
    if meta.dim() != 2 or meta.shape[1] != 4 or not (0 <= count <= meta.shape[0]):
        raise ValueError(f"{who}: meta must be [rows, 4] with count <= rows")


def bank_retention_keys(meta, count: int, now: float) -> torch.Tensor:
    """fp32 [count]: ``strength * expf(-(now - timestamp) / 3600)`` of rows [0, count) -- the part of the recall
    score that belongs to the row alone, and the key of the ``'weakest'`` overflow policy."""
    _check_meta(meta, count, "bank_retention_keys")
    out = torch.empty(count, dtype=torch.float32, device=meta.device)
    check(lib().aura_bank_retention_keys(_p(meta), count, now, _p(out), _stream()), "aura_bank_retention_keys")
    return out


def bank_select_weakest(meta, count: int, now: float, cursor: int, n: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The first ``n`` rows (int64 [n]) of the eviction order of rows [0, count) and their keys (fp32 [n]):
    ascending ``(key, (row - cursor) mod count)``, a NaN key first.  The passes over the ``count`` rows are one
    radix select in the library; the n selected entries are then ordered by one ``torch.sort`` of their
    64-bit composites.  No host sync."""
    _check_meta(meta, count, "bank_select_weakest")
    if not (1 <= n <= count) or cursor < 0:
        raise ValueError(f"bank_select_weakest: need 1 <= n <= count and cursor >= 0 (n={n}, count={count}, cursor={cursor})")
    L = lib()
    nbytes = L.aura_bank_select_weakest_workspace_bytes(count, n)
    if nbytes < 0:
        raise ValueError("bank_select_weakest: unsupported size")
    base = _workspace(meta.device, nbytes)
    slots = torch.empty(n, dtype=torch.int64, device=meta.device)
    keys = torch.empty(n, dtype=torch.float32, device=meta.device)
    check(L.aura_bank_select_weakest(_p(meta), count, now, cursor, n, _p(slots), _p(keys), base, nbytes, _stream()),
          "aura_bank_select_weakest")
    if n == 1:
        return slots, keys
    # (the sort reads the workspace before any later call on this stream can overwrite it)
    order = torch.sort(_workspace_view(meta.device, 8 * n).view(torch.int64)).indices
    return slots[order], keys[order]


QUOTA_MAX_SCOPES = 64


def _scope_list(values, name: str, S: Optional[int] = None) -> np.ndarray:
    a = np.asarray(values, dtype=np.int64).reshape(-1)
    if S is not None and a.size != S:
        raise ValueError(f"{name}: {a.size} entries for {S} scopes")
    return a


def bank_tag_counts(meta, count: int, scope_tags) -> torch.Tensor:
    """int32 [S] (device): how many rows of [0, count) carry each of ``scope_tags`` (host ints in [0, 2^24), distinct
    and ascending; any number of them: 64 per library call).  One upload, no host sync."""
    _check_meta(meta, count, "bank_tag_counts")
    t = _scope_list(scope_tags, "bank_tag_counts")
    if t.size and (np.any(np.diff(t) <= 0) or t[0] < 0 or t[-1] >= TAG_LIMIT):
        raise ValueError("bank_tag_counts: scope_tags must be distinct, ascending and inside [0, 2^24)")
    out = torch.zeros(t.size, dtype=torch.int32, device=meta.device)
    if t.size == 0:
        return out
    tags = torch.from_numpy(t.astype(np.int32)).to(meta.device)
    L = lib()
    for s0 in range(0, t.size, QUOTA_MAX_SCOPES):
        s1 = min(t.size, s0 + QUOTA_MAX_SCOPES)
        check(L.aura_bank_tag_counts(_p(meta), count, tags.data_ptr() + 4 * s0, s1 - s0, out.data_ptr() + 4 * s0,
                                     _stream()), "aura_bank_tag_counts")
    return out


def bank_select_weakest_scoped(meta, count: int, now: float, scope_tags, origins, incoming, quotas,
                               bitmap=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Each scope's own weakest rows (``include/aura_hip.h``, "Per-tag quotas", step 1).  ``scope_tags`` (host ints,
    distinct, ascending), and per scope its tie origin, the number of incoming rows and its quota (host ints; any number
    of scopes: 64 per library call, all calls sharing the bitmap).  Returns ``(packed, bitmap)``, both on the device:
    ``packed`` int64 ``[held (S) | x (S) | slots (T) | composites (T)]`` with ``T = sum(incoming)``, scope s owning the
    entries ``[sum(incoming[:s]), + incoming[s])`` of the last two parts -- its ``x[s]`` victims in arrival order, then
    -1 / INT64_MAX (``scoped_selection_decode`` orders them on the host after THE read); ``bitmap`` int32
    ``[(count + 31) // 32]`` with the victims' bits set on top of what the caller passed in.  One upload, no host sync."""
    _check_meta(meta, count, "bank_select_weakest_scoped")
    t = _scope_list(scope_tags, "scope_tags")
    S = t.size
    o, n_in, q = (_scope_list(v, name, S) for v, name in ((origins, "origins"), (incoming, "incoming"), (quotas, "quotas")))
    if count < 1 or S < 1:
        raise ValueError("bank_select_weakest_scoped: needs a held row and a scope")
    if np.any(np.diff(t) <= 0) or t[0] < 0 or t[-1] >= TAG_LIMIT:
        raise ValueError("bank_select_weakest_scoped: scope_tags must be distinct, ascending and inside [0, 2^24)")
    if np.any(o < 0) or np.any(n_in < 0) or np.any(q < 1) or int(n_in.sum()) > 0x7ffffff0:
        raise ValueError("bank_select_weakest_scoped: origins and incoming must be >= 0, quotas >= 1")
    T = int(n_in.sum())
    i32max = np.iinfo(np.int32).max
    params = np.stack([t, o % count, np.minimum(n_in, i32max), np.minimum(q, i32max)]).astype(np.int32)
    params_d = torch.from_numpy(params).to(meta.device)                         # THE upload: [4, S]
    packed = torch.empty(2 * S + 2 * T, dtype=torch.int64, device=meta.device)
    words = (count + 31) // 32
    if bitmap is None:
        bitmap = torch.zeros(words, dtype=torch.int32, device=meta.device)
    else:
        _need(bitmap, "bitmap", torch.int32)
        if bitmap.numel() < words or bitmap.device != meta.device:
            raise ValueError("bank_select_weakest_scoped: bitmap must hold count bits on meta's device")
    L = lib()
    off = np.concatenate([[0], np.cumsum(n_in)])
    pp, base_p = params_d.data_ptr(), packed.data_ptr()
    for s0 in range(0, S, QUOTA_MAX_SCOPES):
        s1 = min(S, s0 + QUOTA_MAX_SCOPES)
        nbytes = L.aura_bank_select_weakest_scoped_workspace_bytes(count, s1 - s0)
        if nbytes < 0:
            raise ValueError("bank_select_weakest_scoped: unsupported size")
        ws = _workspace(meta.device, nbytes)
        cap = int(off[s1] - off[s0])
        check(L.aura_bank_select_weakest_scoped(
            _p(meta), count, now, pp + 4 * s0, pp + 4 * (S + s0), pp + 4 * (2 * S + s0), pp + 4 * (3 * S + s0), s1 - s0,
            cap, base_p + 8 * s0, base_p + 8 * (S + s0), base_p + 8 * (2 * S + int(off[s0])),
            base_p + 8 * (2 * S + T + int(off[s0])), _p(bitmap), ws, nbytes, _stream()),
            "aura_bank_select_weakest_scoped")
    return packed, bitmap


def scoped_selection_decode(packed, incoming):
    """``packed`` of ``bank_select_weakest_scoped`` on the HOST -> ``(held int64 [S], x int64 [S], victims)``:
    ``victims[s]`` the scope's ``x[s]`` rows in its eviction order (ascending composites)."""
    p = packed.numpy() if isinstance(packed, torch.Tensor) else np.asarray(packed)
    n_in = np.asarray(incoming, dtype=np.int64).reshape(-1)
    S, T = n_in.size, int(n_in.sum())
    held, x = p[:S].copy(), p[S:2 * S].copy()
    slots, comp = p[2 * S:2 * S + T], p[2 * S + T:2 * S + 2 * T]
    victims, o = [], 0
    for s in range(S):
        m = int(n_in[s])
        order = np.argsort(comp[o:o + m], kind="stable")[:int(x[s])]
        victims.append(slots[o:o + m][order].astype(np.int64))
        o += m
    return held, x, victims


def bank_select_weakest_masked(meta, count: int, now: float, cursor: int, n: int, bitmap) -> Tuple[torch.Tensor, torch.Tensor]:
    """``bank_select_weakest`` among the rows whose bit in ``bitmap`` (int32 ``[(count + 31) // 32]``, device) is clear;
    ``n`` must not exceed their number (entries beyond it come back as row -1).  No host sync."""
    _check_meta(meta, count, "bank_select_weakest_masked")
    _need(bitmap, "bitmap", torch.int32)
    if not (1 <= n <= count) or cursor < 0:
        raise ValueError(f"bank_select_weakest_masked: need 1 <= n <= count and cursor >= 0 (n={n}, count={count}, cursor={cursor})")
    if bitmap.numel() < (count + 31) // 32 or bitmap.device != meta.device:
        raise ValueError("bank_select_weakest_masked: bitmap must hold count bits on meta's device")
    L = lib()
    nbytes = L.aura_bank_select_weakest_masked_workspace_bytes(count, n)
    if nbytes < 0:
        raise ValueError("bank_select_weakest_masked: unsupported size")
    base = _workspace(meta.device, nbytes)
    slots = torch.full((n,), -1, dtype=torch.int64, device=meta.device)
    keys = torch.zeros(n, dtype=torch.float32, device=meta.device)
    _workspace_view(meta.device, 8 * n).view(torch.int64).fill_(torch.iinfo(torch.int64).max)   # unfilled: sorted last
    check(L.aura_bank_select_weakest_masked(_p(meta), count, now, cursor, n, _p(bitmap), _p(slots), _p(keys), base, nbytes,
                                            _stream()), "aura_bank_select_weakest_masked")
    if n == 1:
        return slots, keys
    order = torch.sort(_workspace_view(meta.device, 8 * n).view(torch.int64)).indices
    return slots[order], keys[order]


def bank_reinforce(meta, count: int, rows, amount: float, cap: float = 1.0) -> None:
    """``meta[r][0] = min(meta[r][0] + amount, cap)`` where it is below ``cap``, once for every distinct row id
    of ``rows`` (int32, any shape) inside [0, count); ``-1`` and other ids outside are ignored."""
    _check_meta(meta, count, "bank_reinforce")
    _need(rows, "rows", torch.int32)
    if not (amount >= 0.0) or cap != cap:
        raise ValueError("bank_reinforce: amount must be >= 0 and cap a number")
    if rows.device != meta.device:
        raise ValueError("bank_reinforce: rows and meta are on different devices")
    L = lib()
    nbytes = L.aura_bank_reinforce_workspace_bytes(count)
    base = _workspace(meta.device, nbytes)
    check(L.aura_bank_reinforce(_p(meta), count, _p(rows), rows.numel(), amount, cap, base, nbytes, _stream()),
          "aura_bank_reinforce")


REPLAY_PRIORITIES = {"key": 0, "strength": 1, "uniform": 2}
REPLAY_MAX_TAGS = 64
REPLAY_MAX_ALPHA = 16.0


def replay_scope_tags(tags) -> np.ndarray:
    """``tags`` of a replay (None = any tag, an int, or several ints taken as a union; 0 = the untagged rows) as a
    sorted int32 array of distinct tags (empty = any); raises ``ValueError`` for a tag outside ``[0, 2^24)`` or more
    than ``REPLAY_MAX_TAGS`` distinct ones."""
    if tags is None:
        return np.zeros(0, dtype=np.int32)
    if isinstance(tags, torch.Tensor):
        tags = tags.detach().cpu().numpy()
    t = np.asarray(tags)
    if t.dtype.kind not in "iu":
        raise ValueError(f"replay: tags must be integers, got dtype {t.dtype}")
    t = np.unique(t.astype(np.int64).reshape(-1))
    if t.size == 0:
        raise ValueError("replay: an empty tag list (None means any tag)")
    if t[0] < 0 or t[-1] >= (1 << 24):
        raise ValueError("replay: tags must be inside [0, 2^24)")
    if t.size > REPLAY_MAX_TAGS:
        raise ValueError(f"replay: at most {REPLAY_MAX_TAGS} distinct tags per call, got {t.size}")
    return np.ascontiguousarray(t.astype(np.int32))


def _replay_args(who: str, priority, alpha, tags, newer_than, older_than, min_strength, seed, draw):
    """The checked arguments both replay ops hand to the library, from ``priority`` to ``draw`` (the tag array is
    host memory and must outlive the call: the caller keeps the tuple)."""
    if priority not in REPLAY_PRIORITIES:
        raise ValueError(f"{who}: priority must be 'key', 'strength' or 'uniform', got {priority!r}")
    alpha = float(alpha)
    if not (0.0 <= alpha <= REPLAY_MAX_ALPHA):
        raise ValueError(f"{who}: alpha must be in [0, {REPLAY_MAX_ALPHA:g}], got {alpha}")
    t = replay_scope_tags(tags)
    cond, bounds = 0, []
    for bit, v, name in ((1, newer_than, "newer_than"), (2, older_than, "older_than"), (4, min_strength, "min_strength")):
        v32 = 0.0
        if v is not None:
            v32 = float(np.float32(v))
            if v32 != v32:
                raise ValueError(f"{who}: {name} must be a number")
            cond |= bit
        bounds.append(v32)
    seed, draw = int(seed), int(draw)
    if not (0 <= seed < (1 << 64)) or not (0 <= draw < (1 << 64)):
        raise ValueError(f"{who}: seed and draw must be in [0, 2^64)")
    return (REPLAY_PRIORITIES[priority], alpha, t.ctypes.data if t.size else None, t.size, cond, *bounds, seed, draw), t


def bank_replay_keys(meta, count: int, now: float, *, priority: str = "key", alpha: float = 1.0, tags=None,
                     newer_than: Optional[float] = None, older_than: Optional[float] = None,
                     min_strength: Optional[float] = None, seed: int = 0, draw: int = 0,
                     return_uniforms: bool = False):
    """fp32 [count]: the draw key ``d = alpha * lw - log(-log(u))`` of every row of [0, count) for ``(seed, draw)``,
    ``-inf`` for a row that is not eligible (the rule: ``include/aura_hip.h``, "Replay") -- the read-only half of
    ``bank_replay``, whose sample is the top ``n`` of these by ``(d descending, row ascending)``.
    ``return_uniforms``: also int32 [count], the 23-bit integers ``x >> 9`` with ``u = (that + 0.5) * 2^-23``."""
    _check_meta(meta, count, "bank_replay_keys")
    args, keep = _replay_args("bank_replay_keys", priority, alpha, tags, newer_than, older_than, min_strength, seed, draw)
    out = torch.empty(count, dtype=torch.float32, device=meta.device)
    out_u = torch.empty(count, dtype=torch.int32, device=meta.device) if return_uniforms else None
    check(lib().aura_bank_replay_keys(_p(meta), count, now, *args, _p(out), _p(out_u), _stream()),
          "aura_bank_replay_keys")
    del keep
    return (out, out_u) if return_uniforms else out


def bank_replay(meta, count: int, now: float, n: int, *, priority: str = "key", alpha: float = 1.0, tags=None,
                newer_than: Optional[float] = None, older_than: Optional[float] = None,
                min_strength: Optional[float] = None, seed: int = 0,
                draw: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """A seeded draw of ``n`` eligible rows of [0, count) without replacement, the likelier the larger
    ``exp(alpha * lw)`` -> ``(rows int32 [n], keys fp32 [n], eligible int64 scalar)``, all on the device: the first
    ``min(n, eligible)`` eligible rows by ``(d descending, row ascending)`` in that order, then ``-1`` / ``-inf``.
    ``priority``: ``'key'`` (``lw`` = log of the retention key, strength x recency), ``'strength'`` or ``'uniform'``;
    ``tags``: None (any), an int or several (a union; 0 = untagged); the other scope conditions as in
    ``knn_search_scoped``.  The key pass and the radix selection run in the library; the n entries are then ordered
    by one ``torch.sort`` of their composites.  No host sync: the padding is written on the device."""
    _check_meta(meta, count, "bank_replay")
    n = int(n)
    if not (1 <= n <= count):
        raise ValueError(f"bank_replay: need 1 <= n <= count (n={n}, count={count})")
    args, keep = _replay_args("bank_replay", priority, alpha, tags, newer_than, older_than, min_strength, seed, draw)
    L = lib()
    nbytes = L.aura_bank_replay_workspace_bytes(count, n)
    if nbytes < 0:
        raise ValueError("bank_replay: unsupported size")
    base = _workspace(meta.device, nbytes)
    rows = torch.empty(n, dtype=torch.int32, device=meta.device)
    keys = torch.empty(n, dtype=torch.float32, device=meta.device)
    eligible = torch.empty(1, dtype=torch.int64, device=meta.device)
    check(L.aura_bank_replay(_p(meta), count, now, *args, n, _p(rows), _p(keys), _p(eligible), base, nbytes, _stream()),
          "aura_bank_replay")
    del keep
    if n > 1:
        # (the sort reads the workspace before any later call on this stream can overwrite it)
        order = torch.sort(_workspace_view(meta.device, 8 * n).view(torch.int64)).indices
        rows, keys = rows[order], keys[order]
    return rows, keys, eligible[0]


CONSOLIDATE_MAX_BATCH = 1024
CONSOLIDATE_MAX_IMAGE_DIM = 768


def find_repeats(bank, inv_norm, count: int, feats, tau: float, image=None, image_rows=None,
                 n_image: Optional[int] = None, rho=None, lists_flag=None, rho16=None):
    """Which rows of the batch ``feats`` (fp32 [n, D], n <= 1024) repeat a row of ``bank[:count]`` or an earlier row of
    the batch, at cosine >= ``tau`` (the rule in full: ``include/aura_hip.h``) ->
    ``(stored_target int32 [n], batch_leader int32 [n], cos fp32 [n], packed int32 [3 n + 2])``.  The three results are
    views of ``packed``; ``packed[3 n]`` is the call's overflow flag (non-zero: a survivor list of the image scan
    overflowed, the results are incomplete -- repeat without an image) and ``packed[3 n + 1]`` a copy of
    ``lists_flag`` (int32 [1], device; 0 without one), so that ONE device-to-host read of ``packed`` brings the
    results and both flags.  ``image``: a current bf16 image of the normalised rows -- the row-ordered shadow
    (``image_rows`` None) or the list-sorted shadow with ``image_rows = sorted_rows`` and ``n_image = n_sorted`` --
    with ``rho`` as ``bank_shadow_update`` leaves it; None: the dense fp32 scan.  A float16 image (the list-sorted image
    as ``HippocampalFormation`` keeps it) goes with its ``rho16``; without one the bound is derived from ``rho``
    (``half_image_rho_bound``).  No host sync."""
    return _find_repeats(bank, inv_norm, count, feats, tau, image, image_rows, n_image, rho, lists_flag, None, None,
                         rho16)


def find_repeats_scoped(bank, inv_norm, meta, count: int, feats, tags, tau: float, image=None, image_rows=None,
                        n_image: Optional[int] = None, rho=None, lists_flag=None, rho16=None):
    """``find_repeats`` within tags (``aura_bank_find_repeats`` by tag; the rule: ``include/aura_hip.h``): a held row is
    eligible for batch row i only when ``int(meta[r, 3]) == tags[i]``, an in-batch pair only when both rows carry the
    same tag; tag 0 is a scope like any other, a tag outside ``[0, 2^24)`` matches nothing (that row is kept).  ``meta``:
    the bank's metadata (fp32 [rows, 4]); ``tags``: int32 [n] on the bank's device.  Same validation, same four results
    and ``packed`` layout, same image arguments and flags as ``find_repeats``; the cost is that call's plus one 4-byte
    load per surviving pair.  No host sync."""
    if meta is None or tags is None:
        raise ValueError("find_repeats_scoped: meta and tags are required")
    return _find_repeats(bank, inv_norm, count, feats, tau, image, image_rows, n_image, rho, lists_flag, meta, tags,
                         rho16)


def _find_repeats(bank, inv_norm, count, feats, tau, image, image_rows, n_image, rho, lists_flag, meta, tags,
                  rho16=None):
    _need(bank, "bank", torch.float32); _need(inv_norm, "inv_norm", torch.float32); _need(feats, "feats", torch.float32)
    if bank.dim() != 2 or not (0 <= count <= bank.shape[0]) or inv_norm.numel() != bank.shape[0]:
        raise ValueError("find_repeats: bank must be [rows, D] with count <= rows and one inv_norm per row")
    M, D = bank.shape
    if feats.dim() != 2 or feats.shape[1] != D:
        raise ValueError(f"find_repeats: feats must be [n, {D}]")
    n = feats.shape[0]
    if n > CONSOLIDATE_MAX_BATCH:
        raise ValueError(f"find_repeats: at most {CONSOLIDATE_MAX_BATCH} rows per call, got {n}")
    tau = float(tau)
    if not (0.0 < tau <= 1.0):
        raise ValueError(f"find_repeats: tau must be in (0, 1], got {tau}")
    if not (1 <= D <= 4096):
        raise ValueError(f"find_repeats: D={D} must be in [1, 4096]")
    if feats.device != bank.device or inv_norm.device != bank.device:
        raise ValueError("find_repeats: tensors are on different devices")
    ni = 0
    fmt = _lib.IMAGE_BF16
    if image is not None:
        fmt = _need_image(image, "image")
        if fmt == _lib.IMAGE_F16:               # the half image's own residuals, or a bound derived from the bf16 ones
            rho = _need(rho16, "rho16", torch.float32) if rho16 is not None else \
                half_image_rho_bound(_need(rho, "rho", torch.float32), D)
        _need(rho, "rho", torch.float32)
        if D % 8 or D > CONSOLIDATE_MAX_IMAGE_DIM or image.dim() != 2 or image.shape[1] != D or rho.numel() != M:
            raise ValueError("find_repeats: an image needs D % 8 == 0, D <= 768, [rows, D] bf16 and one rho per bank row")
        if image_rows is None:
            ni = count if n_image is None else int(n_image)
            if ni != count or image.shape[0] < count:
                raise ValueError("find_repeats: a row-ordered image holds exactly the first count rows")
        else:
            _need(image_rows, "image_rows", torch.int32)
            ni = image_rows.numel() if n_image is None else int(n_image)
            if not (0 <= ni <= min(image_rows.numel(), image.shape[0])):
                raise ValueError("find_repeats: n_image exceeds the image")
        if image.device != bank.device or rho.device != bank.device or \
                (image_rows is not None and image_rows.device != bank.device):
            raise ValueError("find_repeats: tensors are on different devices")
    elif image_rows is not None:
        raise ValueError("find_repeats: image_rows without an image")
    if meta is not None:
        _check_meta(meta, count, "find_repeats_scoped")
        _need(tags, "tags", torch.int32)
        if meta.shape[0] != M or tags.dim() != 1 or tags.numel() != n:
            raise ValueError(f"find_repeats_scoped: meta must be [{M}, 4] and tags int32 [{n}]")
        if meta.device != bank.device or tags.device != bank.device:
            raise ValueError("find_repeats_scoped: tensors are on different devices")
    packed = torch.zeros(3 * n + 2, dtype=torch.int32, device=bank.device)
    stored, leader, cos = packed[:n], packed[n:2 * n], packed[2 * n:3 * n].view(torch.float32)
    if lists_flag is not None:
        _need(lists_flag, "lists_flag", torch.int32)
        packed[3 * n + 1:].copy_(lists_flag.reshape(-1)[:1])
    if n == 0:
        return stored, leader, cos, packed
    L = lib()
    nbytes = L.aura_bank_find_repeats_workspace_bytes(n)
    if nbytes < 0:
        raise ValueError("find_repeats: unsupported size")
    base = _workspace(bank.device, nbytes)
    check(L.aura_bank_find_repeats(_p(bank), _p(inv_norm), count, D, _p(image), _p(image_rows), ni, _p(rho), _p(feats),
                                   n, tau, _p(stored), _p(leader), _p(cos), _p(packed[3 * n:]), base, nbytes, _p(meta),
                                   _p(tags), fmt, _stream()), "aura_bank_find_repeats")
    return stored, leader, cos, packed


def bank_blend(bank, inv_norm, count: int, stored_target, batch_leader, beta: float, feats=None, out=None,
               feats_row0: int = -1, shadow=None, rho=None, shadow_upto: int = 0, sorted_bf16=None, sorted_rows=None,
               pos_of_row=None, n_sorted: Optional[int] = None, rho16=None) -> None:
    """Blending merges (the rule: ``include/aura_hip.h``, "Blending merges"): every memory that rows of the batch
    repeat moves toward them, ``g = g + beta * (f_i - g)`` over its members in ascending batch order, in one launch.
    ``stored_target`` / ``batch_leader``: int32 [n] on the bank's device, as ONE ``find_repeats`` call against
    ``bank[:count]`` left them (grouping happens on the device; nothing is read back).  ``feats_row0 == -1``: the batch
    is ``feats`` [n, D]; a blended in-batch leader goes to ``out`` [n, D], which the caller has filled with a copy of
    ``feats`` (``feats`` is never written).  ``feats_row0 >= count``: the batch is bank rows
    ``[feats_row0, feats_row0 + n)`` and a blended leader is written in place.  For every BANK row that moves the launch
    also refreshes ``inv_norm`` (``bank_row_norms``' bits), with ``shadow`` + ``rho`` the row's bf16 shadow and residual
    if it lies below ``shadow_upto`` (``bank_shadow_update``'s bits), and with ``sorted_bf16`` + ``sorted_rows`` +
    ``pos_of_row`` (+ ``rho``) its entry of the list-sorted image, in place.  ``rho`` goes with a shadow or an image,
    and only with one; the image's three tensors go together.  The image may be float16 (the dtype is the call's
    ``image_format``); ``rho16``, which goes only with such an image, then receives the half residual while ``rho``
    receives the bf16 one as ever.  Entries out of range are ignored.  No host sync."""
    _need(bank, "bank", torch.float32); _need(inv_norm, "inv_norm", torch.float32)
    _need(stored_target, "stored_target", torch.int32); _need(batch_leader, "batch_leader", torch.int32)
    beta = float(beta)
    if not (0.0 < beta <= 1.0):
        raise ValueError(f"bank_blend: beta must be in (0, 1], got {beta}")
    if bank.dim() != 2 or not (0 <= count <= bank.shape[0]) or inv_norm.numel() != bank.shape[0]:
        raise ValueError("bank_blend: bank must be [rows, D] with count <= rows and one inv_norm per row")
    M, D = bank.shape
    if not (1 <= D <= 4096) or M > 0x7fffffff:
        raise ValueError(f"bank_blend: D={D} must be in [1, 4096] and the bank below 2^31 rows")
    n = stored_target.numel()
    if stored_target.dim() != 1 or batch_leader.shape != stored_target.shape or n > CONSOLIDATE_MAX_BATCH:
        raise ValueError(f"bank_blend: stored_target and batch_leader must be int32 [n], n <= {CONSOLIDATE_MAX_BATCH}")
    feats_row0 = int(feats_row0)
    if feats_row0 == -1:
        if feats is None or out is None:
            raise ValueError("bank_blend: feats and out are required unless the batch is a slab of the bank")
        _need(feats, "feats", torch.float32); _need(out, "out", torch.float32)
        if feats.shape != (n, D) or out.shape != (n, D):
            raise ValueError(f"bank_blend: feats and out must be [{n}, {D}]")
        if out.data_ptr() == feats.data_ptr() and n:
            raise ValueError("bank_blend: out must be a copy of feats, not feats itself")
    else:
        if feats is not None or out is not None:
            raise ValueError("bank_blend: a slab of the bank (feats_row0 >= 0) takes no feats / out")
        if not (count <= feats_row0 and feats_row0 + n <= M):
            raise ValueError(f"bank_blend: the slab [{feats_row0}, {feats_row0 + n}) must lie in [count={count}, {M}]")
    has_image = sorted_bf16 is not None
    if (sorted_rows is not None) != has_image or (pos_of_row is not None) != has_image:
        raise ValueError("bank_blend: sorted_bf16, sorted_rows and pos_of_row go together")
    if (rho is not None) != (shadow is not None or has_image):
        raise ValueError("bank_blend: rho goes with a shadow or a list-sorted image, and only with one")
    if rho is not None:
        _need(rho, "rho", torch.float32)
        if rho.numel() != M or D % 8:
            raise ValueError("bank_blend: a shadow or image needs D % 8 == 0 and one rho per bank row")
    if shadow is not None:
        _need(shadow, "shadow", torch.bfloat16)
        shadow_upto = int(shadow_upto)
        if shadow.shape != bank.shape or not (0 <= shadow_upto <= M):
            raise ValueError("bank_blend: the shadow is [rows, D] bf16 and shadow_upto lies in [0, rows]")
    else:
        shadow_upto = 0
    ns = 0
    fmt = _lib.IMAGE_BF16
    if has_image:
        fmt = _need_image(sorted_bf16, "sorted_bf16"); _need(sorted_rows, "sorted_rows", torch.int32)
        _need(pos_of_row, "pos_of_row", torch.int32)
        ns = sorted_rows.numel() if n_sorted is None else int(n_sorted)
        if sorted_bf16.dim() != 2 or sorted_bf16.shape[1] != D or pos_of_row.numel() != M or \
                not (0 <= ns <= min(sorted_rows.numel(), sorted_bf16.shape[0])):
            raise ValueError("bank_blend: the image is [>= n_sorted, D] bf16 with sorted_rows [>= n_sorted] and "
                             "pos_of_row [rows]")
    if rho16 is not None:
        if fmt != _lib.IMAGE_F16:
            raise ValueError("bank_blend: rho16 goes with a float16 list-sorted image")
        _need(rho16, "rho16", torch.float32)
        if rho16.numel() != M:
            raise ValueError("bank_blend: one rho16 per bank row")
    for t in (inv_norm, stored_target, batch_leader, feats, out, shadow, rho, sorted_bf16, sorted_rows, pos_of_row, rho16):
        if t is not None and t.device != bank.device:
            raise ValueError("bank_blend: tensors are on different devices")
    if n == 0:
        return
    check(lib().aura_bank_blend(_p(bank), _p(inv_norm), count, M, D, _p(feats), feats_row0, n, _p(stored_target),
                                _p(batch_leader), beta, _p(out), _p(shadow), _p(rho), shadow_upto, _p(sorted_bf16),
                                _p(rho16), _p(sorted_rows), _p(pos_of_row), ns, fmt, _stream()), "aura_bank_blend")


def bank_touch(meta, count: int, rows, now: float) -> None:
    """``meta[r][1] = now`` for every row id of ``rows`` (int32, any shape) inside [0, count); others are ignored."""
    _check_meta(meta, count, "bank_touch")
    _need(rows, "rows", torch.int32)
    if rows.device != meta.device:
        raise ValueError("bank_touch: rows and meta are on different devices")
    if now != now:
        raise ValueError("bank_touch: now must be a number")
    check(lib().aura_bank_touch(_p(meta), count, _p(rows), rows.numel(), float(now), _stream()), "aura_bank_touch")


def bank_compact_round_rows() -> int:
    """Rows per round of ``bank_compact`` (the sizes at which its launches change)."""
    return int(lib().aura_bank_compact_round_rows())


def bank_compact(bank, loc, meta, inv_norm, src, dst0: int = 0, shadow=None, rho=None) -> int:
    """In-place compaction: row ``src[i]`` of ``bank`` [rows, D], ``loc`` [rows, S], ``meta`` [rows, 4], ``inv_norm``
    [rows] and -- when given, both or neither -- the row-ordered bf16 ``shadow`` [rows, D] and ``rho`` [rows] moves to
    row ``dst0 + i``, as if every source were read before any destination is written (``include/aura_hip.h``).
    ``src``: a HOST integer array, strictly ascending, ``dst0 + i <= src[i] < rows`` -- checked here with numpy.  The
    leading rows that are in place already are cut off here, the rest is uploaded once: a move that moves nothing
    launches nothing.  Returns the number of rows that change place.  No host sync; the shared workspace."""
    _need(bank, "bank", torch.float32); _need(loc, "loc", torch.float32); _need(meta, "meta", torch.float32)
    _need(inv_norm, "inv_norm", torch.float32)
    if bank.dim() != 2 or loc.dim() != 2 or meta.dim() != 2 or meta.shape[1] != 4:
        raise ValueError("bank_compact: bank [rows, D], loc [rows, S] and meta [rows, 4] expected")
    rows, D = bank.shape
    S = loc.shape[1]
    if loc.shape[0] != rows or meta.shape[0] != rows or inv_norm.numel() != rows:
        raise ValueError("bank_compact: the arrays disagree on the number of rows")
    if (shadow is None) != (rho is None):
        raise ValueError("bank_compact: shadow and rho go together")
    if shadow is not None:
        _need(shadow, "shadow", torch.bfloat16); _need(rho, "rho", torch.float32)
        if shadow.shape != bank.shape or rho.numel() != rows or D % 8:
            raise ValueError("bank_compact: the shadow is [rows, D] bf16 with D % 8 == 0, rho one value per row")
    for t in (loc, meta, inv_norm, shadow, rho):
        if t is not None and t.device != bank.device:
            raise ValueError("bank_compact: tensors are on different devices")
    s = np.ascontiguousarray(np.asarray(src).reshape(-1), dtype=np.int64)
    n, dst0 = s.size, int(dst0)
    if dst0 < 0 or dst0 + n > rows or rows > 0x7fffffff:
        raise ValueError(f"bank_compact: dst0={dst0} and n={n} do not fit {rows} rows")
    if n == 0:
        return 0
    # how far every row moves, plus dst0: src ascends strictly exactly when this never decreases
    shift = s - np.arange(n, dtype=np.int64)
    if s[-1] >= rows or shift[0] < dst0 or (n > 1 and bool((shift[1:] < shift[:-1]).any())):
        raise ValueError("bank_compact: src must ascend strictly with dst0 + i <= src[i] < rows")
    fixed = int(np.searchsorted(shift, dst0, side="right"))       # rows in place already: a prefix
    if fixed == n:
        return 0
    L = lib()
    nbytes = L.aura_bank_compact_workspace_bytes(D, S, 1 if shadow is not None else 0)
    if nbytes < 0:
        raise ValueError(f"bank_compact: unsupported shape D={D}, S={S}")
    base = _workspace(bank.device, nbytes)
    src_t = torch.from_numpy(s[fixed:].astype(np.int32)).to(bank.device)
    check(L.aura_bank_compact(_p(bank), _p(loc), _p(meta), _p(inv_norm), _p(shadow), _p(rho), rows, D, S, _p(src_t),
                              n - fixed, dst0 + fixed, base, nbytes, _stream()), "aura_bank_compact")
    return n - fixed


DIVERSE_MAX_CANDIDATES = 128


def diverse_select(bank, inv_norm, count: int, cand_rows, cand_scores, k: int, diversity: float = 0.0,
                   max_similarity: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Greedy diverse selection of ``k`` rows per query among the ``F`` candidates of a recall (``cand_rows`` int32
    [nq, F] and ``cand_scores`` fp32 [nq, F] in rank order) -> ``(scores [nq, k], rows [nq, k])`` in pick order,
    the candidates' own rows and score bits, ``-inf`` / ``-1`` where fewer than ``k`` were eligible.  A candidate
    whose cosine to an earlier pick reaches ``max_similarity`` is skipped (None: no limit); the others are ranked
    by ``(1 - diversity) * score - diversity * (largest cosine to an earlier pick)``.  The rule in full:
    ``include/aura_hip.h``.  One launch, no host sync."""
    _need(bank, "bank", torch.float32); _need(inv_norm, "inv_norm", torch.float32)
    _need(cand_rows, "cand_rows", torch.int32); _need(cand_scores, "cand_scores", torch.float32)
    if bank.dim() != 2 or not (0 <= count <= bank.shape[0]) or inv_norm.numel() != bank.shape[0]:
        raise ValueError("diverse_select: bank must be [rows, D] with count <= rows and one inv_norm per row")
    M, D = bank.shape
    if cand_rows.dim() != 2 or cand_scores.shape != cand_rows.shape:
        raise ValueError("diverse_select: cand_rows and cand_scores must both be [nq, F]")
    nq, F = cand_rows.shape
    if not (1 <= k <= F <= DIVERSE_MAX_CANDIDATES):
        raise ValueError(f"diverse_select: need 1 <= k <= F <= {DIVERSE_MAX_CANDIDATES} (k={k}, F={F})")
    if D % 4 != 0 or not (4 <= D <= 4096):
        raise ValueError(f"diverse_select: D={D} must be a multiple of 4 in [4, 4096]")
    if not (0.0 <= diversity <= 1.0):
        raise ValueError("diverse_select: diversity must be in [0, 1]")
    tau = 2.0 if max_similarity is None else float(max_similarity)
    if tau != tau:
        raise ValueError("diverse_select: max_similarity must be a number")
    if not (cand_rows.device == cand_scores.device == inv_norm.device == bank.device):
        raise ValueError("diverse_select: tensors are on different devices")
    out_s = torch.empty(nq, k, dtype=torch.float32, device=bank.device)
    out_i = torch.empty(nq, k, dtype=torch.int32, device=bank.device)
    if nq == 0:
        return out_s, out_i
    L = lib()
    nbytes = L.aura_diverse_select_workspace_bytes(nq, F, k)
    if nbytes < 0:
        raise ValueError("diverse_select: unsupported size")
    base = _workspace(bank.device, nbytes)
    check(L.aura_diverse_select(_p(bank), _p(inv_norm), count, D, _p(cand_rows), _p(cand_scores), nq, F, k,
                                float(diversity), tau, _p(out_s), _p(out_i), base, nbytes, _stream()),
          "aura_diverse_select")
    return out_s, out_i


TAG_LIMIT = 1 << 24                 # tags are integers in [0, 2^24): exact as the fp32 of metadata column 3
SCOPED_MAX_K = 128
SCOPED_MAX_SCOPES = 256             # distinct scopes per library call (knn_search_scoped chunks the queries beyond)
SCOPED_MAX_SPLITS = 64
SCOPED_TILE_QUERIES = 64
SCOPED_FLAG_BAD_ROW, SCOPED_FLAG_BAD_PLAN = 1, 2


def bank_set_tags(meta, count: int, slots, tags) -> None:
    """``meta[slots[i]][3] = tags[i]``: the tag stamp of the write paths and of ``retag``.  ``slots`` (int64 [n], device)
    must be distinct and inside [0, count); ``tags`` (int32 [n], device) inside [0, 2^24) -- the callers check both on
    the host, the kernel skips an entry that breaks either.  One launch, no host sync."""
    _check_meta(meta, count, "bank_set_tags")
    _need(slots, "slots", torch.int64); _need(tags, "tags", torch.int32)
    if slots.dim() != 1 or tags.shape != slots.shape:
        raise ValueError("bank_set_tags: slots and tags must both be [n]")
    if slots.device != meta.device or tags.device != meta.device:
        raise ValueError("bank_set_tags: tensors are on different devices")
    if slots.numel() == 0:
        return
    check(lib().aura_bank_set_tags(_p(meta), count, _p(slots), _p(tags), slots.numel(), _stream()), "aura_bank_set_tags")


def scoped_query_tags(tags, nq: int) -> np.ndarray:
    """``tags`` of a scoped recall (None, an int, or one int per query; negative = any tag) as int32 [nq] with every
    "any" entry at -1; raises ``ValueError`` on a length mismatch or a tag >= 2^24."""
    if tags is None:
        return np.full(nq, -1, dtype=np.int32)
    if isinstance(tags, torch.Tensor):
        tags = tags.detach().cpu().numpy()
    t = np.asarray(tags)
    if t.dtype.kind not in "iu":
        raise ValueError(f"tags must be integers, got dtype {t.dtype}")
    t = t.astype(np.int64)
    if t.ndim == 0:
        t = np.full(nq, int(t), dtype=np.int64)
    t = t.reshape(-1)
    if t.size != nq:
        raise ValueError(f"{t.size} tags for {nq} queries")
    if t.size and int(t.max()) >= TAG_LIMIT:
        raise ValueError(f"tags must be below 2^24 = {TAG_LIMIT}, got {int(t.max())}")
    return np.where(t < 0, -1, t).astype(np.int32)


def scoped_plan(qtags: np.ndarray):
    """The plan ``aura_knn_search_scoped`` takes for per-query tags ``qtags`` (int32 [nq], -1 = any):
    ``(plan int32, n_scopes, n_tiles)`` -- the distinct tags ascending, then per tile of at most 64 queries of one
    scope its scope index, first position and length in ``q_order``, then ``q_order`` (the queries grouped by scope,
    in their own order within a scope)."""
    scope_tags, inverse = np.unique(qtags, return_inverse=True)
    order = np.argsort(inverse, kind="stable").astype(np.int32)
    sizes = np.bincount(inverse, minlength=scope_tags.size)
    t_scope, t_q0, t_nq = [], [], []
    q0 = 0
    for s, m in enumerate(sizes.tolist()):
        for lo in range(0, m, SCOPED_TILE_QUERIES):
            t_scope.append(s); t_q0.append(q0 + lo); t_nq.append(min(SCOPED_TILE_QUERIES, m - lo))
        q0 += m
    plan = np.concatenate([scope_tags.astype(np.int32), np.asarray(t_scope, dtype=np.int32),
                           np.asarray(t_q0, dtype=np.int32), np.asarray(t_nq, dtype=np.int32), order])
    return plan, int(scope_tags.size), len(t_scope)


def knn_search_scoped(bank, inv_norm, meta, queries, k: int, now: float, count: int, tags=None,
                      newer_than: Optional[float] = None, older_than: Optional[float] = None,
                      min_strength: Optional[float] = None, loc=None, q_loc=None, check_flag: bool = True,
                      splits: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Exact recall within a scope -> ``(scores [nq, k] fp32, rows [nq, k] int32)``.  Row ``r < count`` is in query
    ``i``'s scope iff ``tags[i] < 0 or int(meta[r][3]) == tags[i]``, ``meta[r][1] >= float32(newer_than)``,
    ``meta[r][1] <= float32(older_than)`` and ``meta[r][0] >= min_strength`` (a condition given as None is not applied);
    the result is the top ``k`` of the scope by the combined score of ``knn_search``, descending, equal scores to the
    lower row, ``-inf`` / ``-1`` where the scope has fewer than ``k`` rows (the rule in full: ``include/aura_hip.h``).
    ``tags``: None (any tag), an int for all queries or one per query (host ints; negative = any; 0 = untagged rows).
    The host sorts and uniques the tags into a plan (one small upload); more than ``SCOPED_MAX_SCOPES`` distinct tags
    are served in several library calls over subsets of the queries -- a pair's score bits do not depend on what
    shares a call.  ``splits`` (default: chosen from the number of query tiles): how many workgroups share a tile's
    row list.  ``check_flag`` reads the call's flag back (one host sync) and raises ``AuraDeviceError`` if a scope
    list held a row outside the bank or the plan was inconsistent."""
    _need(bank, "bank", torch.float32); _need(inv_norm, "inv_norm", torch.float32)
    _need(meta, "meta", torch.float32); _need(queries, "queries", torch.float32)
    if bank.dim() != 2 or queries.dim() != 2 or queries.shape[1] != bank.shape[1]:
        raise ValueError(f"knn_search_scoped: queries must be [nq, {bank.shape[-1]}]")
    M, D = bank.shape
    nq = queries.shape[0]
    count = int(count)
    if not (0 < count <= M) or count >= (1 << 30) or meta.shape != (M, 4) or inv_norm.numel() != M:
        raise ValueError("knn_search_scoped: bad bank/count")
    if not (1 <= D <= 4096):
        raise ValueError(f"knn_search_scoped: D={D} must be in [1, 4096]")
    if not (1 <= k <= min(count, SCOPED_MAX_K)):
        raise ValueError(f"knn_search_scoped: k={k} must be in [1, min(count, {SCOPED_MAX_K})] "
                         f"(a scoped recall returns at most {SCOPED_MAX_K} rows per query)")
    sd = 0
    if q_loc is not None:
        _need(loc, "loc", torch.float32); _need(q_loc, "q_loc", torch.float32)
        sd = loc.shape[1]
        if q_loc.shape != (nq, sd) or loc.shape[0] != M or not (1 <= sd <= 4):
            raise ValueError("knn_search_scoped: location shape mismatch")
    for t in (inv_norm, meta, queries, loc if q_loc is not None else None, q_loc):
        if t is not None and t.device != bank.device:
            raise ValueError("knn_search_scoped: tensors are on different devices")
    qtags = scoped_query_tags(tags, nq)
    cond, bounds = 0, []
    for bit, v, name in ((1, newer_than, "newer_than"), (2, older_than, "older_than"), (4, min_strength, "min_strength")):
        v32 = 0.0
        if v is not None:
            v32 = float(np.float32(v))
            if v32 != v32:
                raise ValueError(f"knn_search_scoped: {name} must be a number")
            cond |= bit
        bounds.append(v32)
    dev = bank.device
    out_s = torch.empty(nq, k, dtype=torch.float32, device=dev)
    out_i = torch.empty(nq, k, dtype=torch.int32, device=dev)
    if nq == 0:
        return out_s, out_i
    L = lib()
    flag = _overflow_flag(dev)

    def run(qt, q, ql, dst_s, dst_i):
        plan, n_scopes, n_tiles = scoped_plan(qt)
        sp = splits
        if sp is None:                    # about 1024 workgroups, no more than the longest possible list has row tiles
            sp = max(1, min(SCOPED_MAX_SPLITS, -(-1024 // n_tiles), -(-count // 128)))
        if not (1 <= sp <= SCOPED_MAX_SPLITS):
            raise ValueError(f"knn_search_scoped: splits must be in [1, {SCOPED_MAX_SPLITS}]")
        n = q.shape[0]
        nbytes = L.aura_knn_scoped_workspace_bytes(count, n, k, n_scopes, sp)
        if nbytes < 0:
            raise ValueError("knn_search_scoped: unsupported size")
        base = _workspace(dev, nbytes)
        plan_t = torch.from_numpy(plan).to(dev)
        check(L.aura_knn_search_scoped(_p(bank), _p(inv_norm), _p(meta), _p(loc) if ql is not None else None, sd, _p(q),
                                       _p(ql), now, count, D, n, k, _p(plan_t), n_scopes, n_tiles, sp, cond, bounds[0],
                                       bounds[1], bounds[2], _p(dst_s), _p(dst_i), base, nbytes, _p(flag), _stream()),
              "aura_knn_search_scoped")
        if check_flag:
            f = int(flag.item())
            if f:
                raise AuraDeviceError(
                    f"aura_knn_search_scoped flagged its call ({f}: "
                    f"{'a scope list held a row outside the bank' if f & SCOPED_FLAG_BAD_ROW else 'an inconsistent plan'})"
                    f": the results are not valid")

    distinct = np.unique(qtags)
    if distinct.size <= SCOPED_MAX_SCOPES:
        run(qtags, queries, q_loc, out_s, out_i)
        return out_s, out_i
    for lo in range(0, distinct.size, SCOPED_MAX_SCOPES):       # many distinct tags: subsets of the queries
        sel = np.nonzero(np.isin(qtags, distinct[lo:lo + SCOPED_MAX_SCOPES]))[0]
        sel_t = torch.from_numpy(sel).to(dev)
        s_part = torch.empty(sel.size, k, dtype=torch.float32, device=dev)
        i_part = torch.empty(sel.size, k, dtype=torch.int32, device=dev)
        run(qtags[sel], queries.index_select(0, sel_t), None if q_loc is None else q_loc.index_select(0, sel_t),
            s_part, i_part)
        out_s[sel_t], out_i[sel_t] = s_part, i_part
    return out_s, out_i


def knn_search(bank, inv_norm, meta, queries, k: int, now: float, count: Optional[int] = None,
               loc=None, q_loc=None, idx_base: int = 0, force_dense: bool = False,
               centroids=None, nprobe: int = 0, check_overflow: bool = True,
               fp32_scan: bool = False, shadow=None, rho=None, return_flag: bool = False):
    """Exact batched recall over rows [0, count) -> (scores [nq, k] fp32, idx [nq, k] int32).

    ``centroids`` (256 x D) + ``nprobe`` switches on the reference's centroid-candidate
    selection.  ``check_overflow`` reads one int back (a host sync) and transparently re-runs the
    dense path if a candidate list overflowed; pass False inside latency-critical loops whose
    data is known to be well behaved.  ``return_flag`` additionally returns the overflow flag
    (int32 [1] on the device) so that a caller can fold the check into a read of its own.
    """
    _need(bank, "bank", torch.float32); _need(inv_norm, "inv_norm", torch.float32)
    _need(meta, "meta", torch.float32); _need(queries, "queries", torch.float32)
    M, D = bank.shape
    N = M if count is None else int(count)
    nq = queries.shape[0]
    if queries.dim() != 2 or queries.shape[1] != D:
        raise ValueError(f"knn_search: queries must be [nq, {D}]")
    if not (0 < N <= M) or meta.shape != (M, 4) or inv_norm.numel() != M:
        raise ValueError("knn_search: bad bank/count")
    if not (0 < k <= min(N, 1024)):
        raise ValueError(f"knn_search: k={k} must be in [1, min(N, 1024)]")
    sd = 0
    if q_loc is not None:
        _need(loc, "loc", torch.float32); _need(q_loc, "q_loc", torch.float32)
        sd = loc.shape[1]
        if q_loc.shape != (nq, sd) or loc.shape[0] != M or sd > 4:
            raise ValueError("knn_search: location shape mismatch")
    if centroids is not None:
        _need(centroids, "centroids", torch.float32)
        if centroids.shape != (256, D) or not (0 < nprobe <= 256):
            raise ValueError("knn_search: centroids must be [256, D]")
    dev = bank.device
    out_s = torch.empty(nq, k, dtype=torch.float32, device=dev)
    out_i = torch.empty(nq, k, dtype=torch.int32, device=dev)
    if nq == 0:
        return (out_s, out_i, torch.zeros(1, dtype=torch.int32, device=dev)) if return_flag else (out_s, out_i)
    L = lib()
    nbytes = L.aura_knn_workspace_bytes(N, nq, k)
    if nbytes < 0:
        raise _lib.AuraHipError("aura_knn_workspace_bytes failed")
    base = _workspace(dev, nbytes)
    ovf = _overflow_flag(dev)

    use_shadow = shadow is not None and q_loc is None
    if use_shadow:
        _need(shadow, "shadow", torch.bfloat16); _need(rho, "rho", torch.float32)
        if shadow.shape != bank.shape or rho.numel() != M:
            raise ValueError("knn_search: shadow must have the bank's shape, rho one entry per row")

    def run(flags):
        if use_shadow:
            check(L.aura_knn_search_shadow(_p(bank), _p(shadow), _p(rho), _p(inv_norm), _p(meta), _p(queries), now,
                                           N, D, nq, k, idx_base, _p(out_s), _p(out_i), base, nbytes,
                                           flags, _p(ovf), _p(centroids), nprobe, _stream()),
                  "aura_knn_search_shadow")
            return
        check(L.aura_knn_search_ex(_p(bank), _p(inv_norm), _p(meta), _p(loc), sd, _p(queries),
                                   _p(q_loc), now, N, D, nq, k, idx_base, _p(out_s), _p(out_i),
                                   base, nbytes, flags, _p(ovf), _p(centroids), nprobe, _stream()),
              "aura_knn_search_ex")

    run(_lib.KNN_FORCE_DENSE if force_dense else (_lib.KNN_FP32_SCAN if fp32_scan else 0))
    if check_overflow and not force_dense and (int(ovf.item()) & ~_lib.KNN_FLAG_NO_CANDIDATES) != 0:
        run(_lib.KNN_FORCE_DENSE)
    return (out_s, out_i, ovf) if return_flag else (out_s, out_i)


def ivf_capacity(longest_lists_total: int, k: int) -> Optional[int]:
    """Candidate slots per query for the IVF recall: the sum of the nprobe longest lists rounded
    up to 2048; None if the two-level select cannot hold it ((cap/2048)*k must be <= 16384)."""
    cap = max(2048, (int(longest_lists_total) + 2047) // 2048 * 2048)
    return cap if (cap // 2048) * k <= 16384 else None


def knn_search_ivf(bank, inv_norm, meta, queries, k: int, now: float, count: int, centroids,
                   nprobe: int, list_rows, list_off, list_len, cap: int, idx_base: int = 0
                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Inverted-list recall over rows [0, count): (scores [nq, k], idx [nq, k], overflow flag [1]).
    The flag is a device tensor (non-zero: some query's probed lists exceed the slot capacity and
    the caller must use the masked full scan); reading it is the caller's decision."""
    _need(bank, "bank", torch.float32); _need(inv_norm, "inv_norm", torch.float32)
    _need(meta, "meta", torch.float32); _need(queries, "queries", torch.float32)
    _need(centroids, "centroids", torch.float32)
    for t, n in ((list_rows, "list_rows"), (list_off, "list_off"), (list_len, "list_len")):
        _need(t, n, torch.int32)
    M, D = bank.shape
    nq = queries.shape[0]
    if queries.dim() != 2 or queries.shape[1] != D or not (0 < count <= M) or meta.shape != (M, 4):
        raise ValueError("knn_search_ivf: shape mismatch")
    if centroids.shape != (256, D) or not (0 < nprobe <= 8):
        raise ValueError("knn_search_ivf: centroids must be [256, D], nprobe in [1, 8]")
    if list_rows.numel() != count or list_off.numel() != 257 or list_len.numel() != 256:
        raise ValueError("knn_search_ivf: list arrays do not match count")
    if not (0 < k <= 1024):
        raise ValueError("knn_search_ivf: k must be in [1, 1024]")
    dev = bank.device
    out_s = torch.empty(nq, k, dtype=torch.float32, device=dev)
    out_i = torch.empty(nq, k, dtype=torch.int32, device=dev)
    ovf = torch.zeros(1, dtype=torch.int32, device=dev) if nq == 0 else _overflow_flag(dev)
    if nq == 0:
        return out_s, out_i, ovf
    L = lib()
    nbytes = L.aura_knn_ivf_workspace_bytes(nq, k, cap)
    if nbytes < 0:
        raise ValueError(f"knn_search_ivf: capacity {cap} is not usable with k={k}")
    base = _workspace(dev, nbytes)
    check(L.aura_knn_search_ivf(_p(bank), _p(inv_norm), _p(meta), _p(queries), now, count, D, nq, k,
                                _p(centroids), nprobe, _p(list_rows), _p(list_off), _p(list_len), cap,
                                idx_base, _p(out_s), _p(out_i), base, nbytes, _p(ovf), _stream()),
          "aura_knn_search_ivf")
    return out_s, out_i, ovf


def ivf2_slack(update_interval: int) -> int:
    """Free entries kept behind every inverted list (a multiple of 16): writes between two centroid
    rebuilds (every ``update_interval`` inserts in the reference) are appended in place."""
    return (min(max(int(update_interval), 64), 512) + 15) // 16 * 16


def ivf2_alloc_rows(max_rows: int, slack: int) -> int:
    """Sorted rows to allocate for a bank of ``max_rows``: every list padded to 16 plus its slack."""
    return (int(max_rows) + 256 * (slack + 16) + 15) // 16 * 16


def ivf2_layout(order, seg_off, slack: int, sorted_rows, pad_off, list_len) -> None:
    """Fill the list-sorted layout (in place, no host sync) from rows grouped by centroid id:
    ``order`` int32 [n] (rows of list c = order[seg_off[c] : seg_off[c+1]]), ``seg_off`` int32 [257].
    ``sorted_rows`` int32 [n_alloc] <- row ids, -1 elsewhere; ``pad_off`` int32 [257] <- list starts
    (multiples of 16, ``slack`` free entries behind every list); ``list_len`` int32 [256]."""
    dev = order.device
    off = seg_off.to(torch.int64)
    lens = off[1:] - off[:-1]
    cap = (lens + slack + 15) // 16 * 16
    po = torch.zeros(257, dtype=torch.int64, device=dev)
    po[1:] = torch.cumsum(cap, 0)
    pad_off.copy_(po.to(torch.int32))
    list_len.copy_(lens.to(torch.int32))
    sorted_rows.fill_(-1)
    n = order.numel()                                          # rows before seg_off[0] have no list
    if n:
        pos = torch.arange(n, device=dev, dtype=torch.int64)
        lid = torch.searchsorted(off[1:].contiguous(), pos, right=True).clamp_(max=255)
        dst = po[lid] + (pos - off[lid])
        listed = pos >= off[0]
        sorted_rows[dst[listed]] = order[listed]


def bank_shadow_sorted(bank, inv_norm, sorted_rows, out, rho, pos_of_row=None, n_sorted: Optional[int] = None,
                       rho16=None) -> None:
    """out[i] = 16-bit shadow row of bank row sorted_rows[i] (zeros where it is -1) for i < n_sorted;
    refreshes rho[row] and the reverse map pos_of_row[row] = i.  ``out`` bf16: the row-ordered shadow's format.
    ``out`` float16: IEEE half, nearest-even, |x| < 2^-14 stored as 0 (no subnormals); ``rho`` still receives the bf16
    residual, bit for bit ``bank_shadow_update``'s, and ``rho16`` (optional) the half image's own."""
    _need(bank, "bank", torch.float32); _need(sorted_rows, "sorted_rows", torch.int32)
    _need(inv_norm, "inv_norm", torch.float32); _need(rho, "rho", torch.float32)
    fmt = _need_image(out, "out")
    if rho16 is not None:
        _need(rho16, "rho16", torch.float32)
        if fmt != _lib.IMAGE_F16 or rho16.numel() != bank.shape[0]:
            raise ValueError("bank_shadow_sorted: rho16 (one per bank row) goes with a float16 image")
    M, D = bank.shape
    n = sorted_rows.numel() if n_sorted is None else int(n_sorted)
    if D % 8 or out.shape[1] != D or not (0 <= n <= min(sorted_rows.numel(), out.shape[0])) or \
            inv_norm.numel() != M or rho.numel() != M:
        raise ValueError("bank_shadow_sorted: shape mismatch")
    if pos_of_row is not None:
        _need(pos_of_row, "pos_of_row", torch.int32)
        if pos_of_row.numel() != M:
            raise ValueError("bank_shadow_sorted: pos_of_row must have one entry per bank row")
    check(lib().aura_bank_shadow_sorted(_p(bank), _p(inv_norm), _p(sorted_rows), _p(out), _p(rho), _p(rho16),
                                        _p(pos_of_row), n, D, fmt, _stream()), "aura_bank_shadow_sorted")


def build_ivf2(bank, inv_norm, cids, slack: int = 0, max_rows: Optional[int] = None, rho=None,
               dtype=torch.float16):
    """Inverted lists in the layout of ``knn_search_ivf2`` for rows [0, n) with centroid ids ``cids``
    (any numeric dtype, < 0: no list): returns a dict with sorted_bf16 (the image; IEEE half unless ``dtype`` is
    torch.bfloat16 -- the key keeps its name), rho, rho16 (the half image's residuals; None for bf16), sorted_rows,
    pad_off, list_len, pos_of_row, flag, n_sorted (sorted rows in use)."""
    if dtype not in (torch.float16, torch.bfloat16):
        raise TypeError("build_ivf2: the image is torch.float16 or torch.bfloat16")
    dev = bank.device
    M, D = bank.shape
    n = cids.numel()
    order, seg_off = group_by_cluster(cids, 256)
    n_alloc = ivf2_alloc_rows(M if max_rows is None else max_rows, slack)
    st = dict(sorted_bf16=torch.empty(n_alloc, D, dtype=dtype, device=dev),
              rho16=torch.zeros(M, dtype=torch.float32, device=dev) if dtype == torch.float16 else None,
              sorted_rows=torch.empty(n_alloc, dtype=torch.int32, device=dev),
              pad_off=torch.zeros(257, dtype=torch.int32, device=dev),
              list_len=torch.zeros(256, dtype=torch.int32, device=dev),
              pos_of_row=torch.full((M,), -1, dtype=torch.int32, device=dev),
              flag=torch.zeros(1, dtype=torch.int32, device=dev),
              rho=torch.zeros(M, dtype=torch.float32, device=dev) if rho is None else rho,
              n_sorted=min(n_alloc, ivf2_alloc_rows(n, slack)), slack=slack)
    ivf2_layout(order, seg_off, slack, st["sorted_rows"], st["pad_off"], st["list_len"])
    bank_shadow_sorted(bank, inv_norm, st["sorted_rows"], st["sorted_bf16"], st["rho"], st["pos_of_row"],
                       st["n_sorted"], rho16=st["rho16"])
    return st


def ivf2_append(bank, inv_norm, meta, slots, sorted_shadow, sorted_rows, pad_off, list_len, pos_of_row, rho,
                flag, row_constants=None, row_constants_now: float = 0.0, rho16=None) -> None:
    """Keep the inverted lists current after a write of the DISTINCT rows ``slots`` (int64 [n]): the
    row's old entry becomes a hole, the row is appended to the list of meta[slot][2].  ``row_constants``
    (``ivf2_row_constants`` for ``row_constants_now``): the cached table follows the touched entries.  A float16
    image takes ``rho16`` beside ``rho`` (required with ``row_constants``: the table is the half image's)."""
    _need(bank, "bank", torch.float32); _need(inv_norm, "inv_norm", torch.float32)
    _need(meta, "meta", torch.float32); _need(slots, "slots", torch.int64)
    fmt = _need_image(sorted_shadow, "sorted_shadow"); _need(rho, "rho", torch.float32)
    if rho16 is not None:
        _need(rho16, "rho16", torch.float32)
        if fmt != _lib.IMAGE_F16 or rho16.numel() != bank.shape[0]:
            raise ValueError("ivf2_append: rho16 (one per bank row) goes with a float16 image")
    elif fmt == _lib.IMAGE_F16 and row_constants is not None:
        raise ValueError("ivf2_append: a float16 image's row constants need rho16")
    for t, n_ in ((sorted_rows, "sorted_rows"), (pad_off, "pad_off"), (list_len, "list_len"),
                  (pos_of_row, "pos_of_row"), (flag, "flag")):
        _need(t, n_, torch.int32)
    M, D = bank.shape
    if sorted_shadow.shape[1] != D or sorted_shadow.shape[0] < sorted_rows.numel() or pad_off.numel() != 257 or \
            list_len.numel() != 256 or pos_of_row.numel() != M or rho.numel() != M or meta.shape != (M, 4) or D % 8:
        raise ValueError("ivf2_append: shape mismatch")
    if row_constants is not None:
        _need(row_constants, "row_constants", torch.float32)
        if row_constants.dim() != 2 or row_constants.shape[1] != 4 or row_constants.shape[0] < sorted_rows.numel():
            raise ValueError("ivf2_append: row_constants must be [>= sorted rows, 4]")
    check(lib().aura_ivf2_append(_p(bank), _p(inv_norm), _p(meta), _p(slots), slots.numel(), D, _p(sorted_shadow),
                                 _p(sorted_rows), _p(pad_off), _p(list_len), _p(pos_of_row), _p(rho), _p(rho16),
                                 _p(flag), _p(row_constants), float(row_constants_now), fmt, _stream()), "aura_ivf2_append")


def ivf2_row_constants(meta, rho, sorted_rows, n_sorted: int, D: int, now: float, out, half: bool = False) -> None:
    """out[i] (fp32 [>= n_sorted, 4]) = the score constants of sorted row i at time ``now`` (see
    ``aura_ivf2_row_constants``): pass ``out`` to ``knn_search_ivf2(row_constants=...)`` for calls with the
    same ``now`` while metadata, rho and the list layout are unchanged.  ``half``: the table of a float16 image --
    ``rho`` is then that image's ``rho16``."""
    _need(meta, "meta", torch.float32); _need(rho, "rho", torch.float32)
    _need(sorted_rows, "sorted_rows", torch.int32); _need(out, "out", torch.float32)
    n = int(n_sorted)
    if out.dim() != 2 or out.shape[1] != 4 or not (0 <= n <= min(out.shape[0], sorted_rows.numel())) or \
            meta.dim() != 2 or meta.shape[1] != 4 or rho.numel() != meta.shape[0]:
        raise ValueError("ivf2_row_constants: shape mismatch")
    fmt = _lib.IMAGE_F16 if half else _lib.IMAGE_BF16
    check(lib().aura_ivf2_row_constants(_p(meta), _p(rho), _p(sorted_rows), n, int(D), float(now), _p(out), fmt, _stream()),
          "aura_ivf2_row_constants")


def centroid_probe(queries, centroids, nprobe: int = 8) -> torch.Tensor:
    """ids [nq, 8] int32: column p < nprobe = the p-th nearest of the 256 centroid rows to each query (L2 on the
    unnormalised query, ``hippocampal.py:261-262``) -- the probes ``knn_search_ivf2`` computes for itself, for callers
    that want them once per query (``sharded.ShardedHippocampus``).  Equal KEYS go to the lower row.  Rows with the
    same bits have equal keys when they sit in one 32-row group (rows [32 w, 32 w + 32) are summed in one order), and
    all-zero rows have everywhere; copies of a row in different groups are summed in different orders once
    64 < D <= 1024 and may then come out in either order, inside the key's rounding bound (tests/index_rule.py)."""
    _need(queries, "queries", torch.float32); _need(centroids, "centroids", torch.float32)
    nq, D = queries.shape
    if centroids.shape != (256, D) or not (0 < nprobe <= 8):
        raise ValueError("centroid_probe: centroids must be [256, D], nprobe in [1, 8]")
    ids = torch.full((nq, 8), -1, dtype=torch.int32, device=queries.device)
    if nq == 0:
        return ids
    L = lib()
    nbytes = L.aura_centroid_probe_workspace_bytes(nq)
    base = _workspace(queries.device, nbytes)
    check(L.aura_centroid_probe(_p(centroids), _p(queries), D, nq, nprobe, _p(ids), base, nbytes, _stream()),
          "aura_centroid_probe")
    return ids


STAGED_MAX_QUERIES = 8192            # queries per staged pass (aura_knn_search_ivf2 with stage != 0)


def knn_search_ivf2(bank, inv_norm, meta, queries, k: int, now: float, centroids, nprobe: int,
                    sorted_shadow, rho, sorted_rows, pad_off, list_len, idx_base: int = 0,
                    n_sorted: Optional[int] = None, lists_flag=None, probe_ids=None, row_constants=None, rho16=None
                    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Inverted-list recall through the two-stage scan: (scores [nq, k], idx [nq, k], overflow flag [1]).
    Same results as ``knn_search_ivf``; the arguments are those of ``Ivf2Lists`` and ``Ivf2Lists.search``.  A float16
    image without ``rho16`` is searched with the bound ``half_image_rho_bound(rho)`` -- rigorous, looser than the
    measured one, and good for this one call only."""
    if rho16 is None and isinstance(sorted_shadow, torch.Tensor) and sorted_shadow.dtype == torch.float16 \
            and row_constants is None:
        rho16 = half_image_rho_bound(_need(rho, "rho", torch.float32), bank.shape[1])
    lists = Ivf2Lists(bank, inv_norm, meta, centroids, nprobe, sorted_shadow, rho, sorted_rows, pad_off, list_len,
                      n_sorted, lists_flag, row_constants, rho16)
    return lists.search(queries, k, now, probe_ids=probe_ids, idx_base=idx_base)


class Ivf2Lists:
    """One layout of the inverted lists that ``knn_search_ivf2`` streams, validated once: the per-call path checks
    only the queries, ``k`` and the probes, allocates the outputs and makes the C call.  (Between a recall's flag
    read and the next recall's first launch the GPU idles; checking the layout on every call cost ~30 us of Python
    -- a dozen tensor checks, ~25 ``data_ptr()`` calls, a workspace-size query -- against a 0.7 ms step.)

    Layout arrays from ``ivf2_layout`` + ``bank_shadow_sorted`` (kept current by ``ivf2_append``).  ``n_sorted``:
    sorted rows in use (a multiple of 16 that covers pad_off[256]; default: all of ``sorted_rows``).
    ``lists_flag``: ``ivf2_append``'s flag; if it is set the returned overflow flag carries ``KNN_FLAG_LISTS_STALE``.
    ``row_constants``: ``ivf2_row_constants`` of the current lists for exactly the ``now`` of every call (fp32).
    The handle keeps its tensors alive and their pointers in ONE ``aura_ivf2_lists`` struct, filled here: a call passes
    the struct's cached address and converts only its own scalars.  An owner rebuilds the handle when ``holds`` fails.
    A float16 ``sorted_shadow`` (IEEE half, ``bank_shadow_sorted``) sets the struct's ``image_format`` and requires
    ``rho16``, that image's residual norms, which the kernels then read in ``rho``'s place (``row_constants`` must be
    the half table, ``ivf2_row_constants(..., half=True)``)."""

    def __init__(self, bank, inv_norm, meta, centroids, nprobe: int, sorted_shadow, rho, sorted_rows, pad_off, list_len,
                 n_sorted: Optional[int] = None, lists_flag=None, row_constants=None, rho16=None):
        _need(bank, "bank", torch.float32); _need(inv_norm, "inv_norm", torch.float32)
        _need(meta, "meta", torch.float32); _need(centroids, "centroids", torch.float32)
        fmt = _need_image(sorted_shadow, "sorted_shadow"); _need(rho, "rho", torch.float32)
        half = fmt == _lib.IMAGE_F16
        for t, n in ((sorted_rows, "sorted_rows"), (pad_off, "pad_off"), (list_len, "list_len")):
            _need(t, n, torch.int32)
        M, D = bank.shape
        if half:
            if rho16 is None:
                raise ValueError("Ivf2Lists: a float16 image needs rho16 (bank_shadow_sorted fills it)")
            _need(rho16, "rho16", torch.float32)
            if rho16.numel() != M:
                raise ValueError("Ivf2Lists: one rho16 per bank row")
        elif rho16 is not None:
            raise ValueError("Ivf2Lists: rho16 goes with a float16 image")
        ns = sorted_rows.numel() if n_sorted is None else int(n_sorted)
        if meta.shape != (M, 4) or rho.numel() != M:
            raise ValueError("Ivf2Lists: shape mismatch")
        if centroids.shape != (256, D) or not (0 < nprobe <= 8):
            raise ValueError("Ivf2Lists: centroids must be [256, D], nprobe in [1, 8]")
        if sorted_shadow.shape[1] != D or not (0 < ns <= min(sorted_rows.numel(), sorted_shadow.shape[0])) or \
                pad_off.numel() != 257 or list_len.numel() != 256 or ns % 16:
            raise ValueError("Ivf2Lists: layout arrays do not match")
        if D % 8 or D > 768:
            raise ValueError("Ivf2Lists: D % 8 == 0, D <= 768")
        if lists_flag is not None:
            _need(lists_flag, "lists_flag", torch.int32)
        if row_constants is not None:
            _need(row_constants, "row_constants", torch.float32)
            if row_constants.dim() != 2 or row_constants.shape[1] != 4 or row_constants.shape[0] < ns:
                raise ValueError("Ivf2Lists: row_constants must be [>= n_sorted, 4]")
        self._keep = (bank, inv_norm, meta, sorted_shadow, rho, sorted_rows, pad_off, list_len, lists_flag, row_constants,
                      centroids, rho16)
        self.M, self.D, self.ns, self.nprobe, self.device = M, D, ns, int(nprobe), bank.device
        self._bytes = {}
        self._lib = lib()
        self.half = half
        # the layout as the C call takes it, filled once: the per-call path passes its address and the call's scalars
        self._struct = _lib.Ivf2ListsStruct(
            bank=_p(bank), inv_norm=_p(inv_norm), meta=_p(meta), centroids=_p(centroids), image=_p(sorted_shadow),
            rho=_p(rho16 if half else rho),                            # the readers take rho16 in rho's place
            sorted_rows=_p(sorted_rows), pad_off=_p(pad_off), list_len=_p(list_len), lists_flag=_p(lists_flag),
            row_constants=_p(row_constants), n_sorted=ns, N=M, D=D, nprobe=self.nprobe, image_format=fmt)
        self._addr = ctypes.addressof(self._struct)

    def holds(self, bank, inv_norm, meta, centroids, nprobe: int, sorted_shadow, rho, sorted_rows, pad_off, list_len,
              n_sorted: Optional[int] = None, lists_flag=None, row_constants=None, rho16=None) -> bool:
        """Whether this handle was built from exactly these tensors (the constructor's arguments)."""
        k = self._keep
        ns = sorted_rows.numel() if n_sorted is None else int(n_sorted)
        return (k[0] is bank and k[1] is inv_norm and k[2] is meta and k[3] is sorted_shadow and k[4] is rho
                and k[5] is sorted_rows and k[6] is pad_off and k[7] is list_len and k[8] is lists_flag
                and k[9] is row_constants and k[10] is centroids and k[11] is rho16 and self.ns == ns
                and self.nprobe == int(nprobe))

    def _call_args(self, queries, k: int, probe_ids):
        """Checks of one call's queries, ``k`` and probes: (nq, probe pointer or None)."""
        if not (isinstance(queries, torch.Tensor) and queries.is_cuda and queries.dtype == torch.float32
                and queries.dim() == 2 and queries.shape[1] == self.D and queries.is_contiguous()):
            _need(queries, "queries", torch.float32)
            raise ValueError(f"Ivf2Lists: queries must be [nq, {self.D}]")
        nq = queries.shape[0]
        if not (0 < k <= 256):
            raise ValueError("Ivf2Lists: k <= 256")
        if probe_ids is None:
            return nq, None
        _need(probe_ids, "probe_ids", torch.int32)
        if tuple(probe_ids.shape) != (nq, 8):
            raise ValueError("Ivf2Lists: probe_ids must be [nq, 8] (centroid_probe)")
        return nq, probe_ids.data_ptr()

    def _scratch(self, nq: int, k: int):
        """(workspace bytes, aligned workspace base, overflow flag, stream) of a call on the current stream."""
        nbytes = self._bytes.get((nq, k))
        if nbytes is None:
            nbytes = self._bytes[(nq, k)] = self._lib.aura_knn_ivf2_workspace_bytes(self.ns, nq, k)
        dev = self.device
        stream = torch.cuda.current_stream(dev).cuda_stream
        key = (dev, stream)
        ws = _workspaces.get(key)
        base = ws[1] if ws is not None and ws[0] >= nbytes else _workspace(dev, nbytes)
        ovf = _ovf_flags.get(key)
        if ovf is None:
            ovf = _overflow_flag(dev)
        return nbytes, base, ovf, stream

    def search(self, queries, k: int, now: float, probe_ids=None, idx_base: int = 0, word=None):
        """(scores [nq, k], idx [nq, k], overflow flag [1]) of ``queries`` fp32 [nq, D].  ``probe_ids``:
        ``centroid_probe``'s output for these queries and this centroid table (the probes are then not recomputed).
        ``word`` (``CompletionWord``): the call's last workgroup also stores the flag there."""
        nq, pid = self._call_args(queries, k, probe_ids)
        dev = self.device
        out_s = torch.empty(nq, k, dtype=torch.float32, device=dev)
        out_i = torch.empty(nq, k, dtype=torch.int32, device=dev)
        if nq == 0:
            if word is not None:
                word.arm(None)
            return out_s, out_i, torch.zeros(1, dtype=torch.int32, device=dev)
        nbytes, base, ovf, stream = self._scratch(nq, k)
        hw, seq = (None, 0) if word is None else (word.ptr, word.arm(ovf))
        check(self._lib.aura_knn_search_ivf2(self._addr, queries.data_ptr(), now, nq, k, pid, idx_base,
                                             out_s.data_ptr(), out_i.data_ptr(), base, nbytes, ovf.data_ptr(), 0, 0, None,
                                             hw, seq, stream), "aura_knn_search_ivf2")
        return out_s, out_i, ovf

    def staged(self, queries, k: int, now: float, probe_ids=None, out=None, idx_base: int = 0) -> "Ivf2Pass":
        """``search`` in stages for one pass of 1..``STAGED_MAX_QUERIES`` queries (see ``Ivf2Pass``).  ``out``:
        (scores [nq, k] fp32, idx [nq, k] int32) to write into (contiguous; e.g. slices of the caller's result)."""
        nq, pid = self._call_args(queries, k, probe_ids)
        if not (0 < nq <= STAGED_MAX_QUERIES):
            raise ValueError("Ivf2Lists.staged: 1..8192 queries per staged pass")
        dev = self.device
        if out is None:
            out = (torch.empty(nq, k, dtype=torch.float32, device=dev), torch.empty(nq, k, dtype=torch.int32, device=dev))
        out_s, out_i = out
        if not (out_s.is_contiguous() and out_i.is_contiguous() and tuple(out_s.shape) == (nq, k)
                and tuple(out_i.shape) == (nq, k) and out_s.dtype == torch.float32
                and out_i.dtype == torch.int32 and out_s.device == dev and out_i.device == dev):
            raise ValueError("Ivf2Lists.staged: out must be contiguous (fp32 [nq, k], int32 [nq, k]) on the bank's device")
        nbytes, base, ovf, _ = self._scratch(nq, k)
        args = (self._addr, queries.data_ptr(), now, nq, k, pid, idx_base, out_s.data_ptr(), out_i.data_ptr(), base,
                nbytes, ovf.data_ptr())
        return Ivf2Pass(self, queries, probe_ids, out_s, out_i, ovf, args)


class Ivf2Pass:
    """One staged pass of ``Ivf2Lists.staged`` (``aura_knn_search_ivf2``, staged): ``stage1(k2)`` -> bounds [nq, 2]
    (the k-th and the k2-th largest sampled lower bound of every query on this bank), ``stage2_bounds(bound [nq], k2)``
    -> the filtered candidates' own bounds [nq, 2], ``stage3(bound2 [nq])`` -> the result re-scored only where a
    candidate can still reach ``bound2``.  Between the calls the caller combines the bounds of all shards of a
    row-sharded bank; nothing else may use this stream's kNN workspace in between."""

    def __init__(self, lists: Ivf2Lists, queries, probe_ids, out_s, out_i, ovf, args: tuple):
        self._keep = (lists, queries, probe_ids)
        self.nq = queries.shape[0]
        self.out_s, self.out_i, self.ovf = out_s, out_i, ovf
        # (a plain tuple, not a closure over self: a self-referencing lambda made every staged pass a reference cycle
        #  that only the cyclic collector freed -- with its 2-MB result views -- and the allocator answered the pile-up
        #  with fresh hipMallocs: recalls of 1.2 ms read 1.6-3.4 ms at random)
        self._args = args

    def _call(self, stage: int, k2: int, bounds) -> None:
        check(self._keep[0]._lib.aura_knn_search_ivf2(*self._args, stage, k2, _p(bounds), None, 0, _stream()),
              "aura_knn_search_ivf2 (staged)")

    def _bound(self, bound: torch.Tensor) -> torch.Tensor:
        _need(bound, "bound", torch.float32)
        if bound.numel() != self.nq:
            raise ValueError("Ivf2Pass: one bound per query")
        return bound

    def stage1(self, k2: int = 0) -> torch.Tensor:
        b = torch.empty(self.nq, 2, dtype=torch.float32, device=self.out_s.device)
        self._call(1, int(k2), b)
        return b

    def stage2_bounds(self, bound: torch.Tensor, k2: int) -> torch.Tensor:
        """Stage 2 up to the filter scan with every threshold raised to ``bound`` first, then the CANDIDATES' bounds
        [nq, 2] (the k-th and the k2-th largest lower bound among this bank's candidates, -inf where there are
        fewer) instead of the refine: for a second, much tighter combination over the shards, consumed by ``stage3``."""
        b = torch.empty(self.nq, 2, dtype=torch.float32, device=self.out_s.device)
        b.view(-1)[: self.nq].copy_(self._bound(bound).reshape(-1))     # in: one bound per query; out: [nq, 2]
        self._call(4, int(k2), b)
        return b

    def stage3(self, bound: torch.Tensor):
        """The refine against a lower bound of every query's k-th best score over ALL shards: candidates whose
        upper bound stays below it are not re-scored (rows of this bank's top k that cannot be in the global top k
        come back as -1).  (scores, idx, overflow flag) as ``search``."""
        self._call(3, 0, self._bound(bound))
        return self.out_s, self.out_i, self.ovf


class CompletionWord:
    """A host-mapped word that receives a recall's flag and a sequence number behind the recall's last launch:
    ``wait()`` polls it -- no device-to-host copy, no stream synchronisation (a blocking wait on a ~1 ms stream costs
    the host 1-2 ms on this runtime).  ``Ivf2Lists.search(word=...)`` fills it from the call's last workgroup
    (``aura_knn_search_ivf2``'s ``host_word``); ``signal(flag)`` enqueues a one-thread launch that copies a flag tensor into
    it (a chain that ends in an entry point without one: the staged recall)."""

    def __init__(self, device):
        self.device = torch.device(device)
        hw = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            check(lib().aura_host_word_alloc(ctypes.byref(hw)), "aura_host_word_alloc")
        self.ptr = hw.value
        self._hw = (ctypes.c_uint32 * 2).from_address(hw.value)
        self._seq = 0
        self._flag = None             # the device flag behind the last launch; None: nothing was launched

    def __del__(self):
        try:
            if getattr(self, "ptr", None):
                torch.cuda.synchronize(self.device)          # no launch may still hold the word
                lib().aura_host_word_free(self.ptr)
                self.ptr = None
        except Exception:
            pass

    def arm(self, flag: Optional[torch.Tensor]) -> int:
        """Record a launch that will fill the word from the device tensor ``flag`` (None: the call launched
        nothing, ``wait`` then reports 0); returns the sequence number that launch has to store."""
        self._flag = flag
        if flag is not None:
            self._seq = (self._seq + 1) & 0x7fffffff or 1
        return self._seq

    def signal(self, flag: torch.Tensor) -> None:
        _need(flag, "flag", torch.int32)
        check(lib().aura_signal_flag(_p(flag), self.ptr, self.arm(flag), _stream()), "aura_signal_flag")

    def wait(self, timeout_s: float = 5.0) -> int:
        """The flag of the last launch (blocks until it has finished)."""
        if self._flag is None:
            return 0
        hw, seq = self._hw, self._seq
        t_end, n = None, 0
        while hw[1] != seq:
            n += 1
            if (n & 0xfff) == 0:                             # every ~4000 polls: give up after timeout_s
                now = time.perf_counter()
                if t_end is None:
                    t_end = now + timeout_s
                elif now > t_end:
                    warnings.warn(f"CompletionWord: no signal after {timeout_s} s; reading the flag from the device")
                    return int(self._flag.item())
        return int(hw[0])


def topk_merge(scores, idx, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """scores, idx: [S, nq, k] per-shard lists -> merged (scores [nq, k], idx [nq, k])."""
    _need(scores, "scores", torch.float32); _need(idx, "idx", torch.int32)
    S, nq, kk = scores.shape
    if idx.shape != scores.shape or kk != k:
        raise ValueError("topk_merge: shape mismatch")
    out_s = torch.empty(nq, k, dtype=torch.float32, device=scores.device)
    out_i = torch.empty(nq, k, dtype=torch.int32, device=scores.device)
    check(lib().aura_topk_merge(_p(scores), _p(idx), S, nq, k, _p(out_s), _p(out_i), _stream()),
          "aura_topk_merge")
    return out_s, out_i


def bank_gather(bank, idx) -> torch.Tensor:
    """rows of ``bank`` at int32 ``idx`` (any shape); indices outside the bank (-1) -> zeros."""
    _need(bank, "bank", torch.float32); _need(idx, "idx", torch.int32)
    D = bank.shape[1]
    n = idx.numel()
    out = torch.empty(*idx.shape, D, dtype=torch.float32, device=bank.device)
    check(lib().aura_bank_gather(_p(bank), bank.shape[0], _p(idx), _p(out), n, D, _stream()), "aura_bank_gather")
    return out


def kmeans_assign(bank, centroids, count: int, k: int) -> torch.Tensor:
    """Nearest of the first k centroids for rows [0, count) -> int32 [count]."""
    _need(bank, "bank", torch.float32); _need(centroids, "centroids", torch.float32)
    M, D = bank.shape
    if not (0 <= count <= M) or centroids.shape[1] != D or not (0 < k <= min(256, centroids.shape[0])):
        raise ValueError("kmeans_assign: shape mismatch")
    assign = torch.empty(count, dtype=torch.int32, device=bank.device)
    ws = torch.empty(256, dtype=torch.float32, device=bank.device)
    check(lib().aura_kmeans_assign(_p(bank), _p(centroids), _p(ws), _p(assign), count, D, k,
                                   _stream()), "aura_kmeans_assign")
    return assign


def group_by_cluster(assign, k: int = 256) -> Tuple[torch.Tensor, torch.Tensor]:
    """Rows grouped by cluster id (stable): (order int32 [n], seg_off int32 [k+1]) with
    order[seg_off[c] : seg_off[c+1]] = rows of cluster c; ids < 0 sort first (seg_off[0] = their
    count).  Device-side sort + bincount, no host sync."""
    a = assign.to(torch.int32)
    order = torch.sort(a, stable=True).indices.to(torch.int32).contiguous()
    valid = a >= 0
    lens = torch.bincount(a.clamp(min=0).long(), weights=valid.to(torch.float32), minlength=k)[:k].to(torch.int64)
    n_neg = (a.numel() - valid.sum()).reshape(1)
    seg_off = torch.cat([n_neg, n_neg + torch.cumsum(lens, 0)]).to(torch.int32).contiguous()
    return order, seg_off


def kmeans_segment_means(bank, order, seg_off, centroids, k: int, sums_only: bool = False) -> None:
    """centroids[c] = mean of bank[order[seg_off[c]:seg_off[c+1]]] for c < k (empty clusters keep theirs);
    ``sums_only``: the sums instead (zeros for empty clusters, also when ``order`` is empty) -- a shard's partial result.
    The summation order is fixed (``aura_hip.h``): the same segment gives the same bits under any id, beside any others."""
    _need(bank, "bank", torch.float32); _need(centroids, "centroids", torch.float32)
    _need(order, "order", torch.int32); _need(seg_off, "seg_off", torch.int32)
    M, D = bank.shape
    N = order.numel()
    if N > M or centroids.shape[1] != D or not (0 < k <= min(256, centroids.shape[0])) or seg_off.numel() < k + 1 or D % 4:
        raise ValueError("kmeans_segment_means: shape mismatch")
    L = lib()
    nbytes = L.aura_kmeans_means_workspace_bytes(N, D, k)
    base = _workspace(bank.device, nbytes)
    check(L.aura_kmeans_segment_means(_p(bank), _p(order), _p(seg_off), _p(centroids), base, nbytes, N, D, k,
                                      1 if sums_only else 0, _stream()), "aura_kmeans_segment_means")


def kmeans_commit(assign, seg_off, meta, counts, k: int) -> None:
    """meta[i][2] = assign[i]; counts[c] = rows of cluster c."""
    _need(assign, "assign", torch.int32); _need(seg_off, "seg_off", torch.int32); _need(meta, "meta", torch.float32)
    N = assign.numel()
    if meta.shape[0] < N or meta.shape[1] != 4 or seg_off.numel() < k + 1 or not (0 < k <= 256):
        raise ValueError("kmeans_commit: shape mismatch")
    if counts is not None:
        _need(counts, "counts", torch.float32)
        if counts.numel() < k:
            raise ValueError("kmeans_commit: counts too small")
    check(lib().aura_kmeans_commit(_p(assign), _p(seg_off), _p(meta), _p(counts), N, k, _stream()),
          "aura_kmeans_commit")


def kmeans_update(bank, assign, centroids, k: int, counts=None, meta=None, update_means: bool = True):
    """One Lloyd update from an assignment: means (``update_means``), counts and metadata ids.
    Returns the grouping (order, seg_off) it used."""
    order, seg_off = group_by_cluster(assign, k)
    if update_means:
        kmeans_segment_means(bank, order, seg_off, centroids, k)
    if meta is not None:
        kmeans_commit(assign, seg_off, meta, counts, k)
    elif counts is not None:
        counts[:k] = (seg_off[1:k + 1] - seg_off[:k]).to(torch.float32)
    return order, seg_off


def addition_linear(x, weight_patterns, bias=None) -> torch.Tensor:
    """-||w_o - x_b||_1 (+ bias): x [B, in], weight_patterns [out, in] -> [B, out]."""
    _need(x, "x", torch.float32); _need(weight_patterns, "weight_patterns", torch.float32)
    if x.dim() != 2 or weight_patterns.dim() != 2 or x.shape[1] != weight_patterns.shape[1]:
        raise ValueError("addition_linear: x must be [B, in] and weights [out, in]")
    if bias is not None:
        _need(bias, "bias", torch.float32)
        if bias.numel() != weight_patterns.shape[0]:
            raise ValueError("addition_linear: bias shape mismatch")
    out = torch.empty(x.shape[0], weight_patterns.shape[0], dtype=torch.float32, device=x.device)
    check(lib().aura_addition_linear(_p(x), _p(weight_patterns), _p(bias), _p(out), x.shape[0],
                                     x.shape[1], weight_patterns.shape[0], _stream()),
          "aura_addition_linear")
    return out


def addition_linear_backward(x, weight_patterns, g_out, need_x: bool = True, need_w: bool = True):
    """Gradients of ``addition_linear``: (g_x [B, in] or None, g_w [out, in] or None); abs -> sign, sign(0) = 0."""
    _need(x, "x", torch.float32); _need(weight_patterns, "weight_patterns", torch.float32)
    _need(g_out, "g_out", torch.float32)
    B, IN = x.shape
    OUT = weight_patterns.shape[0]
    if weight_patterns.shape[1] != IN or tuple(g_out.shape) != (B, OUT):
        raise ValueError("addition_linear_backward: shape mismatch")
    g_x = torch.empty_like(x) if need_x else None
    g_w = torch.empty_like(weight_patterns) if need_w else None
    check(lib().aura_addition_linear_backward(_p(x), _p(weight_patterns), _p(g_out), _p(g_x), _p(g_w), B, IN, OUT,
                                              _stream()), "aura_addition_linear_backward")
    return g_x, g_w
