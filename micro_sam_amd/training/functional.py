"""Differentiable primitives of the mask decoder on libmsam_hip.so (``torch.autograd.Function`` wrappers; torch owns memory,
shapes and the tape, every forward / backward product runs a HIP kernel):

* ``linear``      y = x W^T + b on the MFMA GEMM kernel (``msam_gemm_bf16``), bf16 operands / fp32 accumulation / fp32
                  outputs in BOTH directions: dX = dY W, dW = dY^T X (the reference trains under AMP bf16,
                  ``finetuning/specialists/training/light_microscopy/livecell_multi_gpu_finetuning.py:56-82``); parameters
                  and their gradients stay fp32;
* ``layer_norm``  ``msam_layernorm`` / ``msam_layernorm_backward`` (fp32);
* ``attention``   softmax(q k^T / sqrt(d)) v, ``msam_attention_forward`` / ``msam_attention_backward`` (fp32);
* ``relpos_attention``  the image encoder's attention with its decomposed relative position bias on one token grid,
                  ``msam_relpos_attention_forward`` / ``_backward`` (fp32; gradients also for the two bias tensors).
* ``conv3d_k3``   ``Conv3d(Ci, Co, 3, padding=1)`` on channels-last volumes, ``msam_conv3d_k3_bf16`` in both directions and
                  ``msam_conv3d_k3_wgrad_bf16`` (bf16 operands, fp32 accumulation; the volumetric convolutional decoder);
* ``instance_norm_act``  ``leaky_relu(InstanceNorm3d(a) [+ InstanceNorm3d(r)])``, ``msam_instance_norm_stats`` / ``_apply`` /
                  ``_backward`` (fp32, fp64 sums).

There is no CPU / eager fallback: on a machine without the library these raise.
"""
from __future__ import annotations

import ctypes as C
import math

import os
import weakref

import torch

from .. import _lib, ops


def _pad_to(t: torch.Tensor, rows: int, cols: int) -> torch.Tensor:
    if t.shape[0] == rows and t.shape[1] == cols:
        return t.contiguous()
    out = torch.zeros((rows, cols), dtype=t.dtype, device=t.device)
    out[: t.shape[0], : t.shape[1]] = t
    return out


def _mm_nt(a16: torch.Tensor, b16: torch.Tensor, bias: torch.Tensor = None, n: int = None) -> torch.Tensor:
    """fp32 [M, N] = a16 [M, K] @ b16 [N, K]^T (+ bias [N], fused into the GEMM epilogue) on the MFMA GEMM kernel; K is zero-padded to a
    multiple of 64 and N to a multiple of 128 (the kernel's tile constraints; ``n`` = valid rows of an operand padded beforehand), M is
    arbitrary.  A small output with a very long
    contraction (the weight gradients: M, N <= a few hundred, K = all rows of the batch) is cut into slices of K that run on separate
    workgroups and are added in slice order (``split_k``; the same bits on every run) - two workgroups would otherwise walk the whole
    contraction serially."""
    M, K = a16.shape
    N = b16.shape[0] if n is None else n             # n: rows of b16 that count (b16 already zero-padded to the tile, _weight16)
    K = max(K, b16.shape[1])
    Np = (N + 127) // 128 * 128
    tiles = ((M + 127) // 128) * (Np // 128)
    split = 0
    if bias is None and K >= 8192 and tiles < 128:
        split = 1
        while split * 2 * tiles <= 512 and K // (split * 2) >= 1024:
            split *= 2
    unit = 64 * max(split, 1)
    Kp = (K + unit - 1) // unit * unit
    a = _pad_to(a16, M, Kp)
    b = _pad_to(b16, Np, Kp)
    if bias is not None and Np != N:
        bias = torch.nn.functional.pad(bias.float(), (0, Np - N))
    out = ops.gemm(a, b, None if bias is None else bias.float().contiguous(), out_dtype=torch.float32, split_k=split if split > 1 else 0)
    return out if Np == N else out[:, :N]


# bf16 copies of the weights, W [N, K] and W^T [K, N], per parameter and parameter version: the mask decoder's weights are used by
# 2 images x 8 sub-iterations per optimiser step (reference sam_trainer.py:252-292), the casts and the transposition are the same 16 times
_W16 = {}


def _weight16(weight: torch.Tensor):
    base = weight._base if weight._base is not None else weight
    if not isinstance(base, torch.nn.Parameter):
        w16 = weight.detach().to(torch.bfloat16).contiguous()
        return w16, w16.t().contiguous()
    key = (id(base), tuple(weight.shape), tuple(weight.stride()), weight.storage_offset())
    hit = _W16.get(key)
    stamp = (base._version, base.data_ptr(), base.device.index)       # param.data = ... / .to(device) keep the counter: address + device too
    if hit is not None and hit[0]() is base and hit[1] == stamp:
        return hit[2], hit[3]
    if len(_W16) > 4096:                     # parameters of discarded models
        for k in [k for k, v in _W16.items() if v[0]() is None]:
            del _W16[k]
    w16 = weight.detach().to(torch.bfloat16)
    N, K = w16.shape
    w16t = _pad_to(w16.t(), (K + 127) // 128 * 128, (N + 63) // 64 * 64)          # padded to the product kernel's tiles once, not per call
    w16 = _pad_to(w16, (N + 127) // 128 * 128, (K + 63) // 64 * 64)
    _W16[key] = (weakref.ref(base), stamp, w16, w16t)
    return w16, w16t


def _fusable(t: torch.Tensor) -> bool:
    """msam_cast_transpose takes it: rows contiguous, widths in fours, fp32 or bf16 (everything the model's linears see)."""
    return (t.dim() == 2 and t.stride(1) == 1 and t.shape[1] % 4 == 0 and t.stride(0) % 4 == 0 and t.shape[0] <= 4_000_000
            and t.dtype in (torch.float32, torch.bfloat16) and t.is_cuda and t.data_ptr() % 16 == 0)


class _Linear(torch.autograd.Function):
    """y = x W^T + b.  The weight gradient dW = dY^T X contracts over the rows, and the product kernel wants both operands contiguous
    along the contraction: X^T is written next to the bf16 copy of X in the forward pass, dY^T / the bf16 copy of dY / the bias
    gradient in ONE pass over dY in the backward pass (ops.cast_transpose) - torch's cast + strided transpose copy + sum were 30 % of a
    fine-tuning step (profiles/r03_experiments.md section 8)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        shape = x.shape
        x2 = x.reshape(-1, shape[-1])
        need_dw = weight.requires_grad
        if _fusable(x2):
            a16, a16t, _ = ops.cast_transpose(x2, True, need_dw, False)
        else:
            a16 = x2.to(torch.bfloat16)
            a16t = a16.t().contiguous() if need_dw else None
        w16, w16t = _weight16(weight)
        y = _mm_nt(a16, w16, None if bias is None else bias.detach(), n=weight.shape[0])
        ctx.save_for_backward(a16t if need_dw else None, w16t)
        ctx.has_bias = bias is not None
        ctx.in_shape = shape
        return y.reshape(*shape[:-1], weight.shape[0])

    @staticmethod
    def backward(ctx, dy):
        a16t, w16t = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1])
        want_dw = ctx.needs_input_grad[1] and a16t is not None
        want_db = ctx.has_bias and ctx.needs_input_grad[2]
        if _fusable(dy2):
            dy16, dy16t, db = ops.cast_transpose(dy2, ctx.needs_input_grad[0], want_dw, want_db)
        else:
            dy2 = dy2.contiguous()
            dy16 = dy2.to(torch.bfloat16)
            dy16t = dy16.t().contiguous() if want_dw else None
            db = dy2.float().sum(dim=0) if want_db else None
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = _mm_nt(dy16, w16t, n=ctx.in_shape[-1]).reshape(ctx.in_shape)        # dY [M,N] @ W [N,K]
        if want_dw:
            dw = _mm_nt(dy16t, a16t)                                                 # dY^T [N,M] @ X [M,K]
        return dx, dw, db if want_db else None


def linear(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor = None) -> torch.Tensor:
    return _Linear.apply(x, weight, bias)


# bf16 operands of the depth convolution per parameter and parameter version, as _W16: the tap-major W [Co, 3 Ci] of the forward pass
# and W' [Ci, 3 Co] (taps reversed, channels transposed) of the input gradient, rows zero-padded to the kernel's 128
_WCONV16 = {}


def _conv_weight16(weight: torch.Tensor):
    from .._depthconv import tap_major, tap_major_transposed

    def make():
        w16 = weight.detach().to(torch.bfloat16)
        co, ci = w16.shape[:2]
        return (_pad_to(tap_major(w16), (co + 127) // 128 * 128, 3 * ci), _pad_to(tap_major_transposed(w16), (ci + 127) // 128 * 128, 3 * co))
    if not isinstance(weight, torch.nn.Parameter):
        return make()
    key = id(weight)
    hit = _WCONV16.get(key)
    stamp = (weight._version, weight.data_ptr(), weight.device.index)
    if hit is not None and hit[0]() is weight and hit[1] == stamp:
        return hit[2], hit[3]
    if len(_WCONV16) > 1024:                 # parameters of discarded models
        for k in [k for k, v in _WCONV16.items() if v[0]() is None]:
            del _WCONV16[k]
    w16, w16t = make()
    _WCONV16[key] = (weakref.ref(weight), stamp, w16, w16t)
    return w16, w16t


def _mm_nt_cols(at: torch.Tensor, bt: torch.Tensor, ca: int, cb: int, k: int) -> torch.Tensor:
    """fp32 [Na, Nb] = at[:, ca : ca + k] @ bt[:, cb : cb + k]^T for bf16 ``at`` [Na, M], ``bt`` [Nb, M]: a weight gradient over a RANGE
    of the rows of the batch.  The product kernel takes row strides, so an aligned range is read in place (split-K as ``_mm_nt``: the
    slices are added in order, the same bits on every run); any other range goes through ``_mm_nt`` on copies."""
    na, m = at.shape
    nb = bt.shape[0]
    split = 1
    if k >= 8192:
        tiles = ((na + 127) // 128) * ((nb + 127) // 128)
        while tiles < 128 and split * 2 * tiles <= 512 and k // (split * 2) >= 1024 and k % (128 * split) == 0:
            split *= 2
    if (k % (64 * split) or nb % 128 or m % 8 or ca % 8 or cb % 8 or not at.is_contiguous() or not bt.is_contiguous()
            or at.data_ptr() % 16 or bt.data_ptr() % 16):
        return _mm_nt(at[:, ca:ca + k], bt[:, cb:cb + k])
    out = torch.empty((na, nb), dtype=torch.float32, device=at.device)
    p = _lib.GemmParams()
    p.A, p.lda, p.W, p.ldw, p.M, p.N, p.K = at.data_ptr() + 2 * ca, m, bt.data_ptr() + 2 * cb, m, na, nb, k
    p.out, p.out_dtype, p.ldc = out.data_ptr(), _lib.F32, nb
    p.split_k = split if split > 1 else 0
    _lib.check(_lib.load().msam_gemm_bf16(C.byref(p), _lib.stream_ptr()), "msam_gemm_bf16(rows)")
    return out


class _DepthConv3(torch.autograd.Function):
    """The 3-d adapter's ``Conv3d(Ci, Co, (3, 1, 1), padding="same")`` on token-major rows (csrc/conv3d.hip).  Forward: one
    ``ops.cast_transpose`` of x (its bf16 copy, and X^T if the weight trains), then the kernel.  Backward: one ``ops.cast_transpose`` of
    dY (bf16 copy, dY^T, the column sums = the bias gradient), dX by the SAME kernel on W' (taps reversed, channels transposed), and
    dW per tap = dY^T shift_j(X) on the split-K product kernel over the rows whose tap lies inside the volume: the centre tap over all
    rows at once, an outer tap over D - 1 slices of each volume, the volumes added in index order - the same bits on every run."""

    @staticmethod
    def forward(ctx, x, weight, bias, depth):
        shape = x.shape
        ci, co = int(weight.shape[1]), int(weight.shape[0])
        x2 = x.reshape(-1, ci)
        m = x2.shape[0]
        t = int(shape[1]) * int(shape[2])
        vols = int(shape[0]) // depth
        need_dw = weight.requires_grad
        if _fusable(x2):
            a16, a16t, _ = ops.cast_transpose(x2, True, need_dw, False)
        else:
            a16 = x2.to(torch.bfloat16).contiguous()
            a16t = a16.t().contiguous() if need_dw else None
        w16, w16t = _conv_weight16(weight)
        b = None if bias is None else bias.detach().float().contiguous()
        if b is not None and w16.shape[0] != co:
            b = torch.nn.functional.pad(b, (0, w16.shape[0] - co))
        y = ops.depth_conv3(a16, w16, b, vols, depth, t)
        if w16.shape[0] != co:
            y = y[:, :co]
        ctx.save_for_backward(a16t if need_dw else None, w16t)
        ctx.has_bias = bias is not None
        ctx.geom = (shape, vols, depth, t, m, ci, co)
        return y.reshape(*shape[:-1], co)

    @staticmethod
    def backward(ctx, dy):
        a16t, w16t = ctx.saved_tensors
        shape, vols, depth, t, m, ci, co = ctx.geom
        dy2 = dy.reshape(m, co)
        want_dx = ctx.needs_input_grad[0]
        want_dw = ctx.needs_input_grad[1] and a16t is not None
        want_db = ctx.has_bias and ctx.needs_input_grad[2]
        if _fusable(dy2):
            dy16, dy16t, db = ops.cast_transpose(dy2, want_dx, want_dw, want_db)
        else:
            dy2 = dy2.contiguous()
            dy16 = dy2.to(torch.bfloat16)
            dy16t = dy16.t().contiguous() if want_dw else None
            db = dy2.float().sum(dim=0) if want_db else None
        dx = dw = None
        if want_dx:
            dx = ops.depth_conv3(dy16, w16t, None, vols, depth, t)                   # dX = conv(dY, W')
            if w16t.shape[0] != ci:
                dx = dx[:, :ci]
            dx = dx.reshape(shape)
        if want_dw:
            taps = []
            for j in range(3):
                if j == 1:
                    taps.append(_mm_nt_cols(dy16t, a16t, 0, 0, m))
                    continue
                acc = None
                span = (depth - 1) * t                                               # rows of a volume whose tap j is inside it
                for v in range(vols if span > 0 else 0):
                    r0 = v * depth * t
                    # tap 0 reads the slice before (dY rows from the second slice on), tap 2 the slice after
                    part = _mm_nt_cols(dy16t, a16t, r0 + t, r0, span) if j == 0 else _mm_nt_cols(dy16t, a16t, r0, r0 + t, span)
                    acc = part if acc is None else acc + part
                taps.append(acc if acc is not None else torch.zeros((co, ci), dtype=torch.float32, device=dy.device))
            dw = torch.stack(taps, dim=2).reshape(co, ci, 3, 1, 1)
        return dx, dw, db if want_db else None, None


def depth_conv3(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, depth: int) -> torch.Tensor:
    """``nn.Conv3d(Ci, Co, (3, 1, 1), padding="same")`` along the slices of token-major volumes: x fp32 [B * depth, H, W, Ci] (the
    ``depth`` slices of a volume are consecutive), weight [Co, Ci, 3, 1, 1] (the reference's parameter shape), bias [Co] or None ->
    fp32 [B * depth, H, W, Co].  bf16 operands, fp32 accumulation in both directions; Ci and Co are multiples of 64."""
    if x.dim() != 4 or weight.dim() != 5 or tuple(weight.shape[2:]) != (3, 1, 1) or x.shape[-1] != weight.shape[1]:
        raise ValueError(f"depth_conv3: x must be [B * depth, H, W, Ci] and weight [Co, Ci, 3, 1, 1], got {tuple(x.shape)} and "
                         f"{tuple(weight.shape)}")
    if isinstance(depth, bool) or not isinstance(depth, int) or depth < 1 or x.shape[0] % depth != 0:
        raise ValueError(f"depth_conv3: depth = {depth!r} must be a positive int that divides the {x.shape[0]} slices")
    return _DepthConv3.apply(x, weight, bias, depth)


# bf16 operands of the 3 x 3 x 3 convolution per parameter and parameter version, as _WCONV16: the tap-major W [Co', Kp(Ci)] of the
# forward pass and W' [Ci', Kp(Co)] (taps reversed, channels transposed) of the input gradient, rows zero-padded to the kernel's 16
_WCONV27 = {}


def _conv27_weight16(weight: torch.Tensor):
    from .._conv3d import tap_major, tap_major_transposed

    def make():
        w16 = weight.detach().to(torch.bfloat16)
        return tap_major(w16), tap_major_transposed(w16)
    if not isinstance(weight, torch.nn.Parameter):
        return make()
    key = id(weight)
    hit = _WCONV27.get(key)
    stamp = (weight._version, weight.data_ptr(), weight.device.index)
    if hit is not None and hit[0]() is weight and hit[1] == stamp:
        return hit[2], hit[3]
    if len(_WCONV27) > 1024:                 # parameters of discarded models
        for k in [k for k, v in _WCONV27.items() if v[0]() is None]:
            del _WCONV27[k]
    w16, w16t = make()
    _WCONV27[key] = (weakref.ref(weight), stamp, w16, w16t)
    return w16, w16t


class _Conv3dK3(torch.autograd.Function):
    """``Conv3d(Ci, Co, 3, padding=1)`` on channels-last volumes (csrc/conv3d.hip).  Forward: the bf16 copy of x, then the implicit-GEMM
    kernel.  Backward: the bf16 copy of dY; dX by the SAME kernel on W' (taps reversed, channels transposed); dW by the voxel-contracting
    kernel on the two bf16 copies (no transposed or shifted copy is made); db by the fixed-order column sums of dY (fp32).  Every product
    is one fixed-order sum: the same bits on every run."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        shape = x.shape
        B, D, H, W, ci = (int(v) for v in shape)
        co = int(weight.shape[0])
        a16 = x.reshape(-1, ci).to(torch.bfloat16).contiguous()
        w16, w16t = _conv27_weight16(weight)
        b = None if bias is None else bias.detach().float().contiguous()
        if b is not None and w16.shape[0] != co:
            b = torch.nn.functional.pad(b, (0, w16.shape[0] - co))
        y = ops.conv3d_k3(a16, w16, b, B, D, H, W)
        if w16.shape[0] != co:
            y = y[:, :co]                    # a view: the consumers take a row stride
        ctx.save_for_backward(a16 if weight.requires_grad else None, w16t)
        ctx.has_bias = bias is not None
        ctx.geom = (shape, co)
        return y.view(B, D, H, W, co)        # (splitting the rows of a column slice is still a view)

    @staticmethod
    def backward(ctx, dy):
        a16, w16t = ctx.saved_tensors
        shape, co = ctx.geom
        B, D, H, W, ci = (int(v) for v in shape)
        dy2 = dy.reshape(-1, co)
        want_dx = ctx.needs_input_grad[0]
        want_dw = ctx.needs_input_grad[1] and a16 is not None
        want_db = ctx.has_bias and ctx.needs_input_grad[2]
        dy16 = dy2.to(torch.bfloat16).contiguous() if (want_dx or want_dw) else None
        dx = dw = db = None
        if want_dx:
            dx = ops.conv3d_k3(dy16, w16t, None, B, D, H, W)                        # dX = conv(dY, W')
            if w16t.shape[0] != ci:
                dx = dx[:, :ci]
            dx = dx.reshape(shape)
        if want_dw:
            dw = ops.conv3d_k3_wgrad(a16, dy16, B, D, H, W)
        if want_db:
            d32 = dy2.float()
            wide = 1 << max(2, (co - 1).bit_length())                               # the column sums take a power of two of columns
            if wide != co:
                d32 = torch.nn.functional.pad(d32, (0, wide - co))
            db = ops.column_sums(d32.contiguous() if d32.stride(1) != 1 or d32.stride(0) % 4 else d32)[:co]
        return dx, dw, db


def conv3d_k3(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor = None) -> torch.Tensor:
    """``nn.Conv3d(Ci, Co, 3, padding=1)`` on channels-last volumes: x fp32 [B, D, H, W, Ci], weight [Co, Ci, 3, 3, 3] (the module's
    parameter shape), bias [Co] or None -> fp32 [B, D, H, W, Co].  bf16 operands, fp32 accumulation in both directions; Ci and Co are
    multiples of 8.  (For Co % 16 != 0 the result is a view of the kernel's padded rows.)"""
    if x.dim() != 5 or weight.dim() != 5 or tuple(weight.shape[2:]) != (3, 3, 3) or x.shape[-1] != weight.shape[1]:
        raise ValueError(f"conv3d_k3: x must be [B, D, H, W, Ci] and weight [Co, Ci, 3, 3, 3], got {tuple(x.shape)} and "
                         f"{tuple(weight.shape)}")
    if weight.shape[0] % 8 or weight.shape[1] % 8:
        raise ValueError(f"conv3d_k3: Ci and Co must be multiples of 8, got weight {tuple(weight.shape)}")
    if bias is not None and tuple(bias.shape) != (weight.shape[0],):
        raise ValueError(f"conv3d_k3: bias must be [{weight.shape[0]}], got {tuple(bias.shape)}")
    return _Conv3dK3.apply(x, weight, bias)


def _rows_view(t: torch.Tensor):
    """[B, ..., C] fp32 -> its row matrix [B V, C] without a copy where the rows are evenly strided (a column slice of padded rows)."""
    c = t.shape[-1]
    t = t.float()
    if t.is_contiguous():
        return t.view(-1, c)
    ld = t.stride(-2)
    ok = t.stride(-1) == 1 and ld % 4 == 0 and t.data_ptr() % 16 == 0
    for d in range(t.dim() - 2, 0, -1):
        ok = ok and t.stride(d - 1) == t.stride(d) * t.shape[d]
    if ok:
        return t.as_strided((t.numel() // c, c), (ld, 1))
    return t.contiguous().view(-1, c)


class _InstanceNormAct(torch.autograd.Function):
    """``leaky_relu(instance_norm(a) [+ instance_norm(residual)])`` on channels-last volumes (csrc/conv3d.hip): one statistics pass per
    operand and one fused elementwise pass; backward by its closed form, one statistics pass and one elementwise pass."""

    @staticmethod
    def forward(ctx, a, residual, negative_slope, eps):
        shape = a.shape
        B, c = int(shape[0]), int(shape[-1])
        V = a.numel() // (B * c)
        a2 = _rows_view(a)
        sa = ops.instance_norm_stats(a2, B, V)
        r2 = sr = None
        if residual is not None:
            r2 = _rows_view(residual)
            sr = ops.instance_norm_stats(r2, B, V)
        y, _ = ops.instance_norm_apply(a2, sa, B, V, r2, sr, negative_slope, eps)
        ctx.save_for_backward(a2, sa, r2, sr)
        ctx.conf = (shape, B, V, negative_slope, eps)
        return y.view(shape)

    @staticmethod
    def backward(ctx, dy):
        a2, sa, r2, sr = ctx.saved_tensors
        shape, B, V, negative_slope, eps = ctx.conf
        da, dr = ops.instance_norm_backward(_rows_view(dy), a2, sa, B, V, r2, sr, negative_slope, eps)
        return da.view(shape), None if dr is None else dr.view(shape), None, None


def instance_norm_act(a: torch.Tensor, residual: torch.Tensor = None, negative_slope=0.01, eps: float = 1e-5) -> torch.Tensor:
    """``nn.InstanceNorm3d`` (no affine, no running statistics) of channels-last volumes a [B, D, H, W, C], optionally plus the
    InstanceNorm of ``residual`` (same shape), then ``LeakyReLU(negative_slope)`` (None: no activation) -> fp32 [B, D, H, W, C].  C is a
    power of two in 4 .. 1024; a volume of fewer than 2 voxels raises ``ValueError``."""
    if a.dim() < 3 or (residual is not None and residual.shape != a.shape):
        raise ValueError(f"instance_norm_act: a must be [B, ..., C] and residual of the same shape, got {tuple(a.shape)} and "
                         f"{None if residual is None else tuple(residual.shape)}")
    return _InstanceNormAct.apply(a, residual, negative_slope, eps)


class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        shape = x.shape
        x2 = x.reshape(-1, shape[-1]).float().contiguous()
        y = ops.layernorm(x2, weight.detach().float().contiguous(), bias.detach().float().contiguous(), eps)
        ctx.save_for_backward(x2, weight)
        ctx.eps = eps
        return y.reshape(shape)

    @staticmethod
    def backward(ctx, dy):
        x2, weight = ctx.saved_tensors
        rows, dim = x2.shape
        dy2 = dy.reshape(rows, dim).float().contiguous()
        dx = torch.empty_like(x2)
        dw = torch.zeros((dim,), dtype=torch.float32, device=x2.device)
        db = torch.zeros((dim,), dtype=torch.float32, device=x2.device)
        w = weight.detach().float().contiguous()
        _lib.check(_lib.load().msam_layernorm_backward(x2.data_ptr(), w.data_ptr(), dy2.data_ptr(), float(ctx.eps), rows, dim,
                                                       dx.data_ptr(), dw.data_ptr(), db.data_ptr(), _lib.stream_ptr()),
                   "msam_layernorm_backward")
        return dx.reshape(dy.shape), dw, db, None


def layer_norm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float) -> torch.Tensor:
    """LayerNorm over the last dim (64, 128 or 256 channels; 768 / 1024 / 1280 for the image encoder)."""
    return _LayerNorm.apply(x, weight, bias, eps)


class _Attention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v):
        # q [B, H, Nq, D], k / v [B, H, Nk, D]
        B, H, Nq, D = q.shape
        Nk = k.shape[2]
        qc, kc, vc = q.float().contiguous(), k.float().contiguous(), v.float().contiguous()
        out = torch.empty_like(qc)
        lse = torch.empty((B, H, Nq), dtype=torch.float32, device=q.device)
        scale = 1.0 / math.sqrt(D)
        _lib.check(_lib.load().msam_attention_forward(qc.data_ptr(), kc.data_ptr(), vc.data_ptr(), B * H, Nq, Nk, D, scale,
                                                      out.data_ptr(), lse.data_ptr(), _lib.stream_ptr()), "msam_attention_forward")
        ctx.save_for_backward(qc, kc, vc, out, lse)
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, dout):
        qc, kc, vc, out, lse = ctx.saved_tensors
        B, H, Nq, D = qc.shape
        Nk = kc.shape[2]
        do = dout.float().contiguous()
        dq, dk, dv = torch.empty_like(qc), torch.empty_like(kc), torch.empty_like(vc)
        delta = torch.empty_like(lse)
        _lib.check(_lib.load().msam_attention_backward(qc.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), do.data_ptr(),
                                                       lse.data_ptr(), B * H, Nq, Nk, D, ctx.scale, dq.data_ptr(), dk.data_ptr(),
                                                       dv.data_ptr(), delta.data_ptr(), _lib.stream_ptr()), "msam_attention_backward")
        return dq, dk, dv


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """softmax(q k^T / sqrt(D)) v for q [B, H, Nq, D], k / v [B, H, Nk, D], D in (16, 32)."""
    return _Attention.apply(q, k, v)


class _RelPosAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, bias_h, bias_w, scale):
        # q / k / v [BH, N, D] with N = Gh * Gw tokens of one grid; bias_h [BH, N, Gh], bias_w [BH, N, Gw]
        BH, N, D = q.shape
        Gh, Gw = bias_h.shape[2], bias_w.shape[2]
        if Gh * Gw != N:
            raise ValueError(f"relpos_attention: {N} tokens are not a {Gh} x {Gw} grid")
        qc, kc, vc = q.float().contiguous(), k.float().contiguous(), v.float().contiguous()
        bh, bw = bias_h.float().contiguous(), bias_w.float().contiguous()
        out = torch.empty_like(qc)
        lse = torch.empty((BH, N), dtype=torch.float32, device=q.device)
        _lib.check(_lib.load().msam_relpos_attention_forward(qc.data_ptr(), kc.data_ptr(), vc.data_ptr(), bh.data_ptr(), bw.data_ptr(),
                                                             BH, Gh, Gw, D, float(scale), out.data_ptr(), lse.data_ptr(),
                                                             _lib.stream_ptr()), "msam_relpos_attention_forward")
        ctx.save_for_backward(qc, kc, vc, bh, bw, out, lse)
        ctx.scale = float(scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        qc, kc, vc, bh, bw, out, lse = ctx.saved_tensors
        BH, N, D = qc.shape
        Gh, Gw = bh.shape[2], bw.shape[2]
        do = dout.float().contiguous()
        dq, dk, dv = torch.empty_like(qc), torch.empty_like(kc), torch.empty_like(vc)
        dbh, dbw = torch.empty_like(bh), torch.empty_like(bw)
        delta = torch.empty_like(lse)
        _lib.check(_lib.load().msam_relpos_attention_backward(
            qc.data_ptr(), kc.data_ptr(), vc.data_ptr(), bh.data_ptr(), bw.data_ptr(), out.data_ptr(), do.data_ptr(), lse.data_ptr(),
            BH, Gh, Gw, D, ctx.scale, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dbh.data_ptr(), dbw.data_ptr(), delta.data_ptr(),
            _lib.stream_ptr()), "msam_relpos_attention_backward")
        return dq, dk, dv, dbh, dbw, None


def relpos_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, bias_h: torch.Tensor, bias_w: torch.Tensor,
                     scale: float) -> torch.Tensor:
    """softmax_j(scale q_i k_j + bias_h[i, j // Gw] + bias_w[i, j % Gw]) v for q / k / v [BH, Gh * Gw, D] (D = 64 or 80)."""
    return _RelPosAttention.apply(q, k, v, bias_h, bias_w, scale)


class _SemanticLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, dice_weight, ce_weight, softmax):
        from .._semloss import class_ids
        lc = logits.contiguous()
        tgt = class_ids(target)                                        # (converted once; the backward pass reads the same tensor)
        loss, stats = ops.semantic_loss(lc, tgt, dice_weight, ce_weight, softmax)
        ctx.save_for_backward(lc, tgt, stats.raw)
        ctx.weights = (dice_weight, ce_weight, softmax)
        ctx.mark_non_differentiable(stats.raw)
        return loss, stats.raw

    @staticmethod
    def backward(ctx, dloss, _dstats):
        lc, tgt, raw = ctx.saved_tensors
        dice_weight, ce_weight, softmax = ctx.weights
        # the upstream gradient stays on the device: the kernel reads it there
        up = dloss.to(torch.float32).contiguous()
        return ops.semantic_loss_backward(lc, tgt, raw, up, dice_weight, ce_weight, softmax), None, None, None, None


def semantic_loss(logits: torch.Tensor, target: torch.Tensor, dice_weight: float = 1.0, ce_weight: float = 1.0, softmax: bool = True):
    """Differentiable ``ops.semantic_loss``: ``dice_weight * dice + ce_weight * ce`` of logits [B, C, H, W] against class ids [B, H, W] or
    [B, 1, H, W] in two launches forward and one backward -> (loss, ``ops.SemanticLossStats``; the statistics carry no gradient).
    Logits that are not float32 (bf16 under autocast) are up-cast by autograd's own ``.float()``."""
    from .._semloss import stats_views
    if logits.dtype != torch.float32:
        logits = logits.float()
    loss, raw = _SemanticLoss.apply(logits, target, float(dice_weight), float(ce_weight), bool(softmax))
    return loss, stats_views(raw, int(logits.shape[1]))


# Which implementation the image encoder's attention takes under autograd (training/encoders.py):
#   "gemm"   (default) the two products as plain library batched GEMMs on bf16 operands (torch.bmm = rocBLAS / hipBLASLt on MFMA; what
#            the reference's AMP does), scores + decomposed bias + softmax in fp32 torch operators, backward by autograd.  The score
#            matrix is materialised (24 heads x 4096^2 fp32 = 1.6 GB per global block of vit_b at batch 2: 288 GB of HBM hold it) - the
#            one-thread-per-row fp32 kernels were 34 % of a whole-model step (profiles/r03_train_profile.md);
#   "kernel" the hand-written fp32 kernels (msam_relpos_attention_forward / _backward): no score matrix in HBM, exact fp32, slow -
#            the checked reference of the composite (tests/test_gpu_training_encoders.py) and the low-memory option.
RELPOS_ATTENTION_IMPL = os.environ.get("MSAM_RELPOS_IMPL", "gemm")


def relpos_attention_gemm(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, bias_h: torch.Tensor, bias_w: torch.Tensor,
                          scale: float) -> torch.Tensor:
    BH, N, _ = q.shape
    gh, gw = bias_h.shape[-1], bias_w.shape[-1]
    s = torch.bmm((q * scale).to(torch.bfloat16), k.to(torch.bfloat16).transpose(1, 2)).float()
    s = (s.view(BH, N, gh, gw) + bias_h.unsqueeze(-1) + bias_w.unsqueeze(-2)).view(BH, N, N)
    p = torch.softmax(s, dim=-1)
    return torch.bmm(p.to(torch.bfloat16), v.to(torch.bfloat16)).float()


def relpos_attention_auto(q, k, v, bias_h, bias_w, scale: float) -> torch.Tensor:
    if RELPOS_ATTENTION_IMPL == "gemm":
        return relpos_attention_gemm(q, k, v, bias_h, bias_w, scale)
    return relpos_attention(q, k, v, bias_h, bias_w, scale)
