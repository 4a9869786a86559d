"""The depth convolution of the 3-d adapter (csrc/conv3d.hip, msam_depth_conv3_bf16) restated with torch's own operator:
``torch.nn.Conv3d(Ci, Co, (3, 1, 1), padding="same")`` in fp64 on operands rounded to bf16 - the arithmetic of the reference's
``NDBlockWrapper.adapter_conv`` - plus the case list and the error bounds of tests/test_depth_conv_host.py and
tests/test_gpu_depth_conv.py.

Layouts.  The kernel sees token-major rows, x [B D T, Ci] with row (b D + z) T + t; Conv3d sees [B, Ci, D, T, 1].  The weight is the
module's [Co, Ci, 3, 1, 1]; the kernel's operand is its tap-major form [Co, 3 Ci] (``micro_sam_amd._depthconv.tap_major``).

Inputs.  Every slice (b, z) carries its own large offset (8 .. 8 B D), so that a tap read from the wrong slice or volume - or a tap
that should have been dropped at the end of a volume - moves the output by far more than the tolerance.

Bounds.  A dot product of K terms accumulated in fp32 in ANY order is within K 2^-24 sum |a| |w| of the exact one; doubled for the
final roundings (bias add, store), plus one fp32 ulp of the result: ``2 K 2^-24 sum|a||w| + 2^-23 |out|``."""
import torch

# (B, D, T, Ci, Co)
CASES = [
    (2, 1, 80, 64, 128),         # D = 1: both outer taps vanish everywhere
    (2, 2, 80, 128, 128),        # D = 2
    (2, 3, 80, 384, 384),        # tile rows span slices and the volume boundary; M = 480 is not a multiple of 128
    (1, 5, 128, 384, 384),       # slice = tile
    (3, 2, 200, 64, 256),        # T > tile
]
U = 2.0 ** -24


def r16(t: torch.Tensor) -> torch.Tensor:
    """Rounded to bf16, as fp64."""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def make_case(case, seed: int = 0):
    """-> x [B D T, Ci], weight [Co, Ci, 3, 1, 1], bias [Co], dy [B D T, Co]: fp64 tensors of bf16-representable values (the bias is
    fp32-representable)."""
    B, D, T, Ci, Co = case
    g = torch.Generator().manual_seed(1000 * seed + B + 10 * D + T + Ci + Co)
    off = 8.0 * (1 + torch.arange(B * D, dtype=torch.float64)).reshape(B * D, 1, 1)
    x = r16(torch.randn(B * D, T, Ci, generator=g, dtype=torch.float64) + off).reshape(B * D * T, Ci)
    s = (3 * Ci) ** -0.5
    w = r16(torch.randn(Co, Ci, 3, 1, 1, generator=g, dtype=torch.float64) * s + s)
    bias = (torch.randn(Co, generator=g, dtype=torch.float64) * 3).to(torch.float32).to(torch.float64)
    dy = r16(torch.randn(B * D, T, Co, generator=g, dtype=torch.float64) + off.flip(0)).reshape(B * D * T, Co)
    return x, w, bias, dy


def embed_in_cube(w: torch.Tensor) -> torch.Tensor:
    """[Co, Ci, 3, 1, 1] -> the 3 x 3 x 3 weight [Co, Ci, 3, 3, 3] that holds the depth taps at [:, :, kz, 1, 1] and zeros elsewhere: on a
    volume [B, D, H = T, W = 1] it is the same convolution."""
    cube = w.new_zeros(w.shape[0], w.shape[1], 3, 3, 3)
    cube[:, :, :, 1, 1] = w[:, :, :, 0, 0]
    return cube


def to_volume(rows: torch.Tensor, B: int, D: int, T: int) -> torch.Tensor:
    return rows.reshape(B, D, T, 1, rows.shape[-1]).permute(0, 4, 1, 2, 3)             # [B, C, D, T, 1]


def to_rows(vol: torch.Tensor) -> torch.Tensor:
    return vol.permute(0, 2, 3, 4, 1).reshape(-1, vol.shape[1])


def conv_module(w: torch.Tensor, bias=None) -> torch.nn.Conv3d:
    co, ci = w.shape[:2]
    m = torch.nn.Conv3d(ci, co, kernel_size=(3, 1, 1), padding="same", bias=bias is not None, dtype=torch.float64)
    with torch.no_grad():
        m.weight.copy_(w)
        if bias is not None:
            m.bias.copy_(bias)
    return m


def forward(case, x, w, bias=None):
    """-> (out [M, Co] fp64, the bound per element)."""
    B, D, T, Ci, Co = case
    with torch.no_grad():
        out = to_rows(conv_module(w, bias)(to_volume(x, B, D, T)))
        mag = to_rows(conv_module(w.abs())(to_volume(x.abs(), B, D, T)))
    return out, 2 * 3 * Ci * U * mag + 2.0 ** -23 * out.abs()


def input_gradient(case, dy, w):
    """dX of the convolution for the upstream gradient dy: torch's transpose convolution in fp64 -> (dx [M, Ci], the bound)."""
    B, D, T, Ci, Co = case
    f = torch.nn.functional.conv_transpose3d
    dx = to_rows(f(to_volume(dy, B, D, T), w, padding=(1, 0, 0)))
    mag = to_rows(f(to_volume(dy.abs(), B, D, T), w.abs(), padding=(1, 0, 0)))
    return dx, 2 * 3 * Co * U * mag + 2.0 ** -23 * dx.abs()


def autograd(case, x, w, bias, dy):
    """fp64 autograd of the restatement -> (dx, dw [Co, Ci, 3, 1, 1], db) with their bounds: dX as ``input_gradient``; dW with K = the
    contracted rows of the tap (all M for the centre tap, B (D - 1) T for an outer one); db within M 2^-24 sum |dy|."""
    B, D, T, Ci, Co = case
    xv = to_volume(x, B, D, T).clone().requires_grad_()
    m = conv_module(w, bias)
    (m(xv) * to_volume(dy, B, D, T)).sum().backward()
    mm = conv_module(w.abs(), bias)
    xa = to_volume(x.abs(), B, D, T).clone()
    (mm(xa) * to_volume(dy.abs(), B, D, T)).sum().backward()
    M = B * D * T
    k = torch.tensor([B * (D - 1) * T, M, B * (D - 1) * T], dtype=torch.float64).reshape(1, 1, 3, 1, 1)
    dw, db = m.weight.grad, m.bias.grad
    dx, dx_bound = input_gradient(case, dy, w)
    assert torch.allclose(to_rows(xv.grad), dx, rtol=1e-12, atol=1e-9)                   # the two statements of dX agree
    return (dx, dx_bound), (dw, 2 * k * U * mm.weight.grad + 2.0 ** -23 * dw.abs()), (db, M * U * dy.abs().sum(0))
