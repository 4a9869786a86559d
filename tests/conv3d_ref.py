"""The 3 x 3 x 3 convolution of the volumetric convolutional decoder (csrc/conv3d.hip, msam_conv3d_k3_bf16 / msam_conv3d_k3_wgrad_bf16)
restated with torch's own operators: ``torch.nn.Conv3d(Ci, Co, 3, padding=1)`` in fp64 on operands rounded to bf16, its transpose
convolution and fp64 autograd - plus the case list and the error bounds of tests/test_conv3d_host.py and tests/test_gpu_conv3d.py.

Layouts.  The kernel sees channels-last voxel rows, x [B D H W, Ci] with row ((b D + z) H + y) W + x; Conv3d sees [B, Ci, D, H, W].  The
weight is the module's [Co, Ci, 3, 3, 3]; the kernel's operand is its tap-major form (``micro_sam_amd._conv3d.tap_major``).

Inputs.  Every voxel carries an offset that grows with z, y and x (and with the volume), so that a tap read from the wrong neighbour, from
the next row of the image, from the next slice or from the next volume - or a tap that should have been dropped at a border - moves the
output by far more than the tolerance.

Bounds (the project's).  A dot product of K terms accumulated in fp32 in ANY order is within K 2^-24 sum |a| |w| of the
exact one; doubled for the final roundings (bias add, store), plus one fp32 ulp of the result: ``2 K 2^-24 sum|a||w| + 2^-23 |out|``.
K = 27 Ci forward, 27 Co for dX, the contracted voxel count of the tap for dW; db within M 2^-24 sum |dy|."""
import functools

import torch

# (B, D, H, W, Ci, Co)
CASES = [
    (1, 1, 8, 8, 32, 16),         # D = 1: all 18 off-plane taps vanish
    (2, 3, 5, 7, 16, 8),          # the head's shape: taps mix inside a k-tile, K = 432 padded to 448, Co = 8 padded, M = 210 spans tiles
    (2, 2, 6, 10, 64, 32),
    (1, 3, 9, 4, 256, 128),       # M = 108 < one tile, K = 6912
    (1, 2, 16, 24, 128, 64),      # several M tiles
]
AUTOGRAD_ONLY = (1, 2, 32, 64, 64, 32)   # a weight-gradient contraction of 4096 voxels: the split path
U = 2.0 ** -24


def r16(t: torch.Tensor) -> torch.Tensor:
    """Rounded to bf16, as fp64."""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


@functools.lru_cache(maxsize=None)
def make_case(case, seed: int = 0):
    """-> x [M, Ci], weight [Co, Ci, 3, 3, 3], bias [Co], dy [M, Co]: fp64 tensors of bf16-representable values (the bias is
    fp32-representable).  Cached: the tests share them and leave them unchanged."""
    B, D, H, W, Ci, Co = case
    g = torch.Generator().manual_seed(1000 * seed + B + 10 * D + H + 3 * W + Ci + Co)
    b, z, y, x = torch.meshgrid(*(torch.arange(n, dtype=torch.float64) for n in (B, D, H, W)), indexing="ij")
    off = (2.0 + 1.5 * x + 2.5 * y + 4.0 * z + 6.0 * b).reshape(-1, 1)
    xs = r16(torch.randn(B * D * H * W, Ci, generator=g, dtype=torch.float64) + off)
    s = (27 * Ci) ** -0.5
    w = r16(torch.randn(Co, Ci, 3, 3, 3, generator=g, dtype=torch.float64) * s + s)
    bias = (torch.randn(Co, generator=g, dtype=torch.float64) * 3).to(torch.float32).to(torch.float64)
    dy = r16(torch.randn(B * D * H * W, Co, generator=g, dtype=torch.float64) + off.flip(0))
    return xs, w, bias, dy


def to_volume(rows: torch.Tensor, case) -> torch.Tensor:
    B, D, H, W = case[:4]
    return rows.reshape(B, D, H, W, rows.shape[-1]).permute(0, 4, 1, 2, 3)             # [B, C, D, H, W]


def to_rows(vol: torch.Tensor) -> torch.Tensor:
    return vol.permute(0, 2, 3, 4, 1).reshape(-1, vol.shape[1])


def conv_module(w: torch.Tensor, bias=None) -> torch.nn.Conv3d:
    co, ci = w.shape[:2]
    m = torch.nn.Conv3d(ci, co, kernel_size=3, padding=1, bias=bias is not None, dtype=torch.float64)
    with torch.no_grad():
        m.weight.copy_(w)
        if bias is not None:
            m.bias.copy_(bias)
    return m


def forward(case, x, w, bias=None):
    """-> (out [M, Co] fp64, the bound per element)."""
    Ci = case[4]
    with torch.no_grad():
        out = to_rows(conv_module(w, bias)(to_volume(x, case)))
        mag = to_rows(conv_module(w.abs())(to_volume(x.abs(), case)))
    return out, 2 * 27 * Ci * U * mag + 2.0 ** -23 * out.abs()


def input_gradient(case, dy, w):
    """dX of the convolution for the upstream gradient dy: torch's transpose convolution in fp64 -> (dx [M, Ci], the bound)."""
    Co = case[5]
    f = torch.nn.functional.conv_transpose3d
    dx = to_rows(f(to_volume(dy, case), w, padding=1))
    mag = to_rows(f(to_volume(dy.abs(), case), w.abs(), padding=1))
    return dx, 2 * 27 * Co * U * mag + 2.0 ** -23 * dx.abs()


def tap_counts(case) -> torch.Tensor:
    """[3, 3, 3]: the voxels a tap contracts over (those whose neighbour of the tap lies inside the volume)."""
    B, D, H, W = case[:4]

    def n(size):
        return torch.tensor([size - 1, size, size - 1], dtype=torch.float64)
    return B * n(D).reshape(3, 1, 1) * n(H).reshape(1, 3, 1) * n(W).reshape(1, 1, 3)


@functools.lru_cache(maxsize=None)
def autograd(case):
    """fp64 autograd of the restatement on ``make_case(case)`` -> (dx, dw [Co, Ci, 3, 3, 3], db), each with its bound: dX as
    ``input_gradient``; dW with K = the contracted voxels of the tap; db within M 2^-24 sum |dy|."""
    x, w, bias, dy = make_case(case)
    xv = to_volume(x, case).clone().requires_grad_()
    m = conv_module(w, bias)
    (m(xv) * to_volume(dy, case)).sum().backward()
    mm = conv_module(w.abs(), bias)
    (mm(to_volume(x.abs(), case).clone()) * to_volume(dy.abs(), case)).sum().backward()
    M = x.shape[0]
    k = tap_counts(case).reshape(1, 1, 3, 3, 3)
    dw, db = m.weight.grad, m.bias.grad
    dx, dx_bound = input_gradient(case, dy, w)
    assert torch.allclose(to_rows(xv.grad), dx, rtol=1e-12, atol=1e-9)                   # the two statements of dX agree
    return (dx, dx_bound), (dw, 2 * k * U * mm.weight.grad + 2.0 ** -23 * dw.abs()), (db, M * U * dy.abs().sum(0))
