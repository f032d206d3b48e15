"""Model-input patches in torch tensors: the thin layer between Context.camshift_*_tensor_device and a network's input.

    fmt = PatchFormat.mean_std(mean, std, dtype="f16", layout="chw", channels="rgb")
    x = empty_patches(n, 112, 112, fmt, "cuda")          # [n, 3, 112, 112] float16
    align_sources_into(ctx, x, streams, entries, fmt)    # ONE launch behind the track step
                                                         # (prefilter=8: block-mean patches for large faces, still one launch)
    ctx.synchronize()                                    # or order torch's stream behind ctx.stream
    y = model(x)

THE STREAM RULE.  The work is enqueued on the Context's stream (Context.stream), not on torch's current stream, and nothing here waits.
Before torch reads the tensor the caller either orders torch's stream behind the context's (an event recorded on Context.stream that
torch's stream waits for, or a Context created on torch's stream) or calls Context.synchronize().  The tensor must stay alive until then.

torch is imported in this module only; the rest of the package does not need it."""
from __future__ import annotations

import torch

from .api import PatchFormat

_DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def empty_patches(n: int, width: int, height: int, fmt, device="cuda") -> torch.Tensor:
    """an uninitialised [n, C, H, W] (fmt.layout == "chw") or [n, H, W, C] ("hwc") tensor of fmt's dtype, contiguous"""
    fmt = PatchFormat.of(fmt)
    if n < 1:
        raise ValueError("empty_patches: n must be at least 1")
    return torch.empty((int(n), *fmt.shape(width, height)), dtype=_DTYPES[fmt.dtype], device=device)


def _target(what: str, tensor, n: int, fmt):
    """(data pointer, width, height, stride in bytes) of a tensor a call of n entries may write, or an error that names what is wrong"""
    fmt = PatchFormat.of(fmt)
    if not isinstance(tensor, torch.Tensor):
        raise TypeError(f"{what}: a torch tensor is required")
    if tensor.dtype != _DTYPES[fmt.dtype]:
        raise TypeError(f"{what}: the tensor is {tensor.dtype}, the format says {fmt.dtype}")
    if tensor.dim() != 4 or tensor.shape[0] != n:
        raise ValueError(f"{what}: a tensor of shape [{n}, ...] with four dimensions is required, not {tuple(tensor.shape)}")
    C = fmt.nchannels
    if fmt.layout == "chw":
        c, height, width = (int(v) for v in tensor.shape[1:])
    else:
        height, width, c = (int(v) for v in tensor.shape[1:])
    if c != C or width < 1 or height < 1:
        raise ValueError(f"{what}: {fmt.layout} with {C} channel(s) does not fit a tensor of shape {tuple(tensor.shape)}")
    if not tensor[0].is_contiguous():
        raise ValueError(f"{what}: every patch of the tensor must be contiguous")
    stride = int(tensor.stride(0)) * tensor.element_size() if n > 1 else fmt.default_stride(width, height)
    if stride % 4 or stride < fmt.patch_bytes(width, height):
        raise ValueError(f"{what}: patches must be a multiple of 4 bytes apart and must not overlap (they are {stride} bytes apart)")
    if tensor.data_ptr() % 4:
        raise ValueError(f"{what}: the tensor's data must be 4-byte aligned")
    return tensor.data_ptr(), width, height, stride


def _on_device(what: str, ctx, tensor):
    if not tensor.is_cuda:
        raise ValueError(f"{what}: the tensor must live in device memory, not on {tensor.device}")
    index = tensor.device.index if tensor.device.index is not None else torch.cuda.current_device()
    if index != ctx.device:
        raise ValueError(f"{what}: the tensor lives on device {index}, the context on device {ctx.device}")


def crop_pairs_into(ctx, tensor, pairs, fmt, margin: float = 1.0, square: bool = False, prefilter=None):
    """Context.camshift_crop_pairs_tensor_device into `tensor` (empty_patches(len(pairs), w, h, fmt)): size and stride are the tensor's"""
    ptr, w, h, stride = _target("crop_pairs_into", tensor, len(pairs), fmt)
    _on_device("crop_pairs_into", ctx, tensor)
    if prefilter is not None:  # the block-mean prefilter: max_factor 1..8 (Context.camshift_crop_pairs_filtered_device)
        ctx.camshift_crop_pairs_filtered_device(ptr, pairs, w, h, max_factor=prefilter, fmt=fmt, margin=margin, square=square, stride=stride)
        return
    ctx.camshift_crop_pairs_tensor_device(ptr, pairs, w, h, fmt, margin=margin, square=square, stride=stride)


def crop_sources_into(ctx, tensor, streams, entries, fmt, margin: float = 1.0, square: bool = False, prefilter=None):
    ptr, w, h, stride = _target("crop_sources_into", tensor, len(entries), fmt)
    _on_device("crop_sources_into", ctx, tensor)
    if prefilter is not None:  # the block-mean prefilter: max_factor 1..8 (Context.camshift_crop_sources_filtered_device)
        ctx.camshift_crop_sources_filtered_device(ptr, streams, entries, w, h, max_factor=prefilter, fmt=fmt, margin=margin, square=square, stride=stride)
        return
    ctx.camshift_crop_sources_tensor_device(ptr, streams, entries, w, h, fmt, margin=margin, square=square, stride=stride)


def align_pairs_into(ctx, tensor, pairs, fmt, margin: float = 1.0, square: bool = False, prefilter=None):
    ptr, w, h, stride = _target("align_pairs_into", tensor, len(pairs), fmt)
    _on_device("align_pairs_into", ctx, tensor)
    if prefilter is not None:  # the block-mean prefilter: max_factor 1..8 (Context.camshift_align_pairs_filtered_device)
        ctx.camshift_align_pairs_filtered_device(ptr, pairs, w, h, max_factor=prefilter, fmt=fmt, margin=margin, square=square, stride=stride)
        return
    ctx.camshift_align_pairs_tensor_device(ptr, pairs, w, h, fmt, margin=margin, square=square, stride=stride)


def align_sources_into(ctx, tensor, streams, entries, fmt, margin: float = 1.0, square: bool = False, prefilter=None):
    ptr, w, h, stride = _target("align_sources_into", tensor, len(entries), fmt)
    _on_device("align_sources_into", ctx, tensor)
    if prefilter is not None:  # the block-mean prefilter: max_factor 1..8 (Context.camshift_align_sources_filtered_device)
        ctx.camshift_align_sources_filtered_device(ptr, streams, entries, w, h, max_factor=prefilter, fmt=fmt, margin=margin, square=square, stride=stride)
        return
    ctx.camshift_align_sources_tensor_device(ptr, streams, entries, w, h, fmt, margin=margin, square=square, stride=stride)
