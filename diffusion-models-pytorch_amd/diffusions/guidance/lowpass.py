"""Host tables of ILVR's low-pass filter (reference utils/resize_right/resize_right.py, interp_methods.py).

`resize` is linear and separable: per axis, output o is a weighted sum over `taps` consecutive inputs starting
at `left[o]` of the zero-padded axis, with antialiased (stretched) kernels when downscaling and every row of
weights normalised. The weights depend on torch's float32 rounding of the reference's grid / field-of-view /
weights expressions, so this module evaluates the same torch CPU op sequence (resize_right.py:125-149, 203-213,
342-354) -- its own code, nothing imported from the reference -- once per (size, factor, method), and the
device kernels (csrc/guidance.hip) only apply the tables.
"""
from functools import lru_cache
from math import ceil, pi
from typing import List, Tuple

import torch
from torch import Tensor

_EPS = torch.finfo(torch.float32).eps


def _cubic(x: Tensor) -> Tensor:
    a = torch.abs(x)
    a2 = a ** 2
    a3 = a ** 3
    return ((1.5 * a3 - 2.5 * a2 + 1.) * (a <= 1.).to(x.dtype) +
            (-0.5 * a3 + 2.5 * a2 - 4. * a + 2.) * ((1. < a) & (a <= 2.)).to(x.dtype))


def _lanczos(n: int):
    def f(x: Tensor) -> Tensor:
        return (((torch.sin(pi * x) * torch.sin(pi * x / n) + _EPS) / ((pi ** 2 * x ** 2 / n) + _EPS)) *
                (abs(x) < n).to(x.dtype))
    return f


def _linear(x: Tensor) -> Tensor:
    return (x + 1) * ((-1 <= x) & (x < 0)).to(x.dtype) + (1 - x) * ((0 <= x) & (x <= 1)).to(x.dtype)


def _box(x: Tensor) -> Tensor:
    return ((-1 <= x) & (x < 0)).to(x.dtype) + ((0 <= x) & (x <= 1)).to(x.dtype)


# method -> (kernel, support size)
INTERP_METHODS = {
    'cubic': (_cubic, 4), 'lanczos2': (_lanczos(2), 4), 'lanczos3': (_lanczos(3), 6), 'linear': (_linear, 2),
    'box': (_box, 1),
}


def axis_table(in_sz: int, out_sz: int, scale: float, method: str) -> Tuple[Tensor, Tensor]:
    """(weights [out_sz, taps] float32, left [out_sz] int32) of one resized axis; left indexes the unpadded
    axis (taps outside [0, in_sz) meet the zero padding)."""
    kernel, support = INTERP_METHODS[method]
    scale = float(scale)
    # projected grid: output pixel centres in input coordinates
    grid = torch.arange(out_sz) / scale + (in_sz - 1) / 2 - (out_sz - 1) / (2 * scale)
    if scale < 1.0:  # antialiasing: the kernel stretched by 1 / scale
        base = kernel
        kernel = lambda arg: scale * base(scale * arg)  # noqa: E731
        support = support / scale
    # field of view
    left = (grid - support / 2 - _EPS).ceil().long()
    fov = left[:, None] + torch.arange(ceil(support - _EPS))
    # the reference shifts grid and field of view by the left padding before it takes the distances
    pad = -fov[0, 0].item()
    fov = fov + pad
    grid = grid + pad
    w = kernel(grid[:, None] - fov)
    s = w.sum(1, keepdim=True)
    s[s == 0] = 1
    w = w / s
    return w.to(torch.float32).contiguous(), (fov[:, 0] - pad).to(torch.int32).contiguous()


@lru_cache(maxsize=64)
def axis_tables(H: int, W: int, N: int, method: str) -> List[Tuple[Tensor, Tensor]]:
    """The four tables of low_pass_filter on H x W planes at factor N, in pass order: down-H, down-W, up-H, up-W."""
    if method not in INTERP_METHODS:
        raise ValueError(f'Invalid interp_method: {method} (options: {sorted(INTERP_METHODS)})')
    if N < 1 or H % N != 0 or W % N != 0:
        raise ValueError(f'downsample_factor {N} must divide the image size {H} x {W}')
    down = 1. / N
    # the reference's output sizes: ceil(scale * size), which float rounding may push past size / N
    if ceil(down * H) != H // N or ceil(down * W) != W // N:
        raise ValueError(f'downsample_factor {N}: 1 / {N} times {H} x {W} does not round to {H // N} x {W // N}')
    return [axis_table(H, H // N, down, method), axis_table(W, W // N, down, method),
            axis_table(H // N, H, N, method), axis_table(W // N, W, N, method)]


def densify(table: Tuple[Tensor, Tensor], in_sz: int, dtype=torch.float64) -> Tensor:
    """The [out, in_sz] matrix of a table (taps in the padding dropped)."""
    w, left = table
    out, taps = w.shape
    m = torch.zeros((out, in_sz), dtype=dtype)
    for o in range(out):
        for k in range(taps):
            i = int(left[o]) + k
            if 0 <= i < in_sz:
                m[o, i] += w[o, k].to(dtype)
    return m
