"""The AdaptFormer branch kernel (csrc/adapter.hip, msam_adapter_bf16) restated in fp64, with the case list and the error bound of
tests/test_adapter_host.py and tests/test_gpu_adapter.py:

    out = x + y + alpha (relu(y Wd^T + bd) Wu^T + bu)

The reference takes operands that already hold 16-bit values (y, Wd, Wu; bd, bu, alpha and x hold fp32 values) and does NOT round the
hidden: the kernel's one rounding of it is part of the bound.

Bound, per output element (r, c), with h the exact hidden, u = 2^-9 (bf16) or 2^-12 (fp16) and U = 2^-24:

    |alpha| sum_p |Wu[c, p]| (u |h_p| + (D + 2) U (sum_k |y_k| |Wd[p, k]| + |bd_p|))            the hidden as the kernel holds it
      + (P + 4) U (|alpha| (sum_p |Wu[c, p]| |h_p| + |bu_c|) + |x| + |y|)                          the second product and the final adds

* a dot product of K terms accumulated in fp32 in any order is within K U sum |a| |w| of the exact one; the bias add and the slack of the
  magnitude itself make it (D + 2) U;
* ReLU is 1-Lipschitz: the hidden's error passes through unamplified; its rounding to the 16-bit type adds u |h|;
* the second product has K = P terms, then the bias add, the multiplication by alpha, the add of y and the add of x: (P + 4) U of the
  magnitudes.
The bound is derived, not measured; the tests print worst error / bound (at most 0.89 on these cases, host build and device).

Its u is half of the formats' unit roundoff (bf16 has 8 significand bits: 2^-8; fp16 2^-11), so it is not a worst case for arbitrarily many
elements: over the 2 M elements of a (16383, 128, 64) problem, run once on the host build, 6 elements exceeded it, by up to 1.105 x, each by
exactly what rounding the EXACT hidden to bf16 once gives (0.0056124 at row 139, column 3).  The cases below stay inside it."""
import functools

import torch

# (R, D, P): a single row; a ragged tail below and above one tile; the three model widths' divisibility classes; the largest hidden
CASES = [(1, 128, 32), (17, 128, 64), (129, 768, 64), (257, 1280, 64), (64, 256, 128)]
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
UNIT = {"bf16": 2.0 ** -9, "fp16": 2.0 ** -12}
U = 2.0 ** -24
ALPHA = 0.75


def r16(t: torch.Tensor, dtype: str) -> torch.Tensor:
    """Rounded to the 16-bit type, as fp64."""
    return t.to(torch.float32).to(DTYPES[dtype]).to(torch.float64)


def r32(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32).to(torch.float64)


@functools.lru_cache(maxsize=None)
def make_case(case, dtype: str, seed: int = 0):
    """-> dict of fp64 tensors: y [R, D], wd [P, D], wu [D, P] of 16-bit values; bd [P], bu [D], x [R, D] of fp32 values.  Cached: the
    tests share them and leave them unchanged.  y is LayerNorm-like (unit variance), the pre-activations have zero mean: about half of
    the hidden is clipped by the ReLU."""
    R, D, P = case
    g = torch.Generator().manual_seed(7919 * seed + 31 * R + 7 * D + P + (0 if dtype == "bf16" else 1))

    def rn(*shape):
        return torch.randn(*shape, generator=g, dtype=torch.float64)
    return dict(y=r16(rn(R, D), dtype), wd=r16(rn(P, D) * D ** -0.5, dtype), bd=r32(rn(P) * 0.5),
                wu=r16(rn(D, P) * P ** -0.5, dtype), bu=r32(rn(D)), x=r32(rn(R, D) * 3.0))


def hidden(y, wd, bd):
    """The exact hidden relu(y Wd^T + bd) and the magnitude sum_k |y_k| |Wd[p, k]| + |bd_p| of its pre-activation."""
    return torch.relu(y @ wd.T + bd), y.abs() @ wd.abs().T + bd.abs()


def forward(y, wd, bd, wu, bu, x, alpha: float, dtype: str):
    """-> (out [R, D] fp64, the bound per element)."""
    D, P = wu.shape
    h, mag = hidden(y, wd, bd)
    out = x + y + alpha * (h @ wu.T + bu)
    a = abs(alpha)
    first = a * ((UNIT[dtype] * h + (D + 2) * U * mag) @ wu.abs().T)
    second = (P + 4) * U * (a * (h @ wu.abs().T + bu.abs()) + x.abs() + y.abs())
    return out, first + second


def zero_fraction(y, wd, bd) -> float:
    return float((hidden(y, wd, bd)[0] == 0).double().mean())
