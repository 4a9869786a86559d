"""The InstanceNorm of the volumetric convolutional decoder (csrc/conv3d.hip: msam_instance_norm_stats / _apply / _backward) restated with
torch's own operators - ``F.instance_norm`` (no affine, eps = 1e-5) of one or two operands, their sum, ``F.leaky_relu(0.01)`` - in fp64,
plus the shapes, the inputs and the yardstick of tests/test_instnorm_host.py and tests/test_gpu_instnorm.py.

Layout.  The kernels see channels-last rows [B V, C]; ``F.instance_norm`` sees [B, C, V].

Inputs.  fp32 values with a mean of about 100 per channel (a different one per channel) against unit spread: a one-pass
``E[x^2] - E[x]^2`` in fp32 would lose every digit of the variance.  The residual is correlated with ``a`` so that the sum of the two
normalised operands stays away from the kink of the activation (asserted), where a gradient has no bound.

Yardstick (the project's convention).  torch's own fp32 composite on the same inputs against the fp64 values; the
kernels may be at most 4 times as far (largest absolute error), with floors of 2 fp32 ulps of the largest output and 2^-22 of the largest
gradient.  The bf16 output is compared with the ROUNDED fp64 value, within one bf16 ulp."""
import functools

import torch
import torch.nn.functional as F

SHAPES = [(2, 2, 8), (1, 105, 16), (2, 3000, 128)]          # (B, V, C)
EPS, SLOPE = 1e-5, 0.01


@functools.lru_cache(maxsize=None)
def make(shape):
    """-> a, r, dy: fp32 [B V, C].  Cached: shared by the tests, left unchanged."""
    B, V, C = shape
    g = torch.Generator().manual_seed(B + 10 * V + 1000 * C)
    off = 100.0 + 3.0 * torch.arange(C, dtype=torch.float64) / C
    a = (torch.randn(B * V, C, generator=g, dtype=torch.float64) + off).float()
    noise = torch.randn(B * V, C, generator=g, dtype=torch.float64) * (0.3 if V > 2 else 0.0)
    r = (0.7 * a.double() + noise + 30.0).float()                      # a mean of about 100 as well
    dy = torch.randn(B * V, C, generator=g, dtype=torch.float64).float()
    return a, r, dy


def composite(shape, a, r, act: bool):
    """[B V, C] rows (any float dtype; r may be None) -> leaky_relu(IN(a) + IN(r)) as rows, by torch."""
    B, V, C = shape

    def norm(t):
        return F.instance_norm(t.reshape(B, V, C).permute(0, 2, 1), eps=EPS).permute(0, 2, 1).reshape(B * V, C)
    y = norm(a) if r is None else norm(a) + norm(r)
    return F.leaky_relu(y, SLOPE) if act else y


@functools.lru_cache(maxsize=None)
def reference(shape, with_r: bool, act: bool):
    """-> dict: y (fp64), da, dr (fp64 autograd for the upstream ``make(shape)[2]``; dr None without a residual) and the allowed largest
    absolute errors tol_y, tol_g from torch's fp32 composite."""
    a, r, dy = make(shape)

    def run(dtype):
        aa = a.to(dtype).clone().requires_grad_()
        rr = r.to(dtype).clone().requires_grad_() if with_r else None
        y = composite(shape, aa, rr, act)
        (y * dy.to(dtype)).sum().backward()
        return y.detach(), aa.grad, (rr.grad if with_r else None)
    y, da, dr = run(torch.float64)
    if act:
        assert float(y.abs().min()) > 1e-9                              # away from the kink
    y32, da32, dr32 = run(torch.float32)
    grads = [(da, da32)] + ([(dr, dr32)] if with_r else [])
    yard_y = float((y32.double() - y).abs().max())
    yard_g = max(float((g32.double() - g).abs().max()) for g, g32 in grads)
    gmax = max(float(g.abs().max()) for g, _ in grads)
    return dict(y=y, da=da, dr=dr, yard_y=yard_y, yard_g=yard_g, tol_y=max(4 * yard_y, 2 * 2.0 ** -23 * float(y.abs().max())),
                tol_g=max(4 * yard_g, 2.0 ** -22 * gmax))


def bf16_check(y16: torch.Tensor, y64: torch.Tensor) -> float:
    """Largest |y16 - round_bf16(y64)| in bf16 ulps of the value (asserted <= 1)."""
    want = y64.float().to(torch.bfloat16).double()
    ulp = torch.maximum(2.0 ** (torch.floor(torch.log2(y64.abs().clamp_min(1e-30))) - 7), torch.tensor(2.0 ** -133, dtype=torch.float64))
    worst = float(((y16.double() - want).abs() / ulp).max())
    assert worst <= 1.0, worst
    return worst


CONFIGS = [(False, False), (False, True), (True, False), (True, True)]      # (with residual, with activation)
