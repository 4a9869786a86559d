"""The accepted cases of the tensor -> pointer boundary (tests/test_ops_boundary_host.py) on the device, against fp64, and one
refusal per tensor argument of every wrapper for a CPU tensor among device tensors.

Bounds: a 16-bit output of an op that also has an fp32 output equals, bit for bit, the fp32 output of the same call rounded to
nearest-even in that type (the kernels round the same fp32 value: ``pack16`` / ``f2h`` of csrc/common.h is the compiler's
``(_Float16)`` conversion, round-to-nearest-even).  Against fp64: the bound of the op's fp32 test (tests/test_gpu_kernels.py
test_layernorm 2e-5 + 1e-5 |ref|, test_gemm_plain 1e-3 + 1e-4 |ref|) plus half an ulp of fp16, 2^-11 |ref|.  The row-strided
``cast_transpose`` equals the call on the ``.contiguous()`` copy bit for bit.

The refusals run with the recorder of the host file in place of the library: whatever a wrapper would hand over is noted, nothing
can be launched, so a missing check shows as a recorded call and never as a kernel reading a host address.

The value tests take a ``dev`` fixture: the host file runs the same bodies against the host-compiled library."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def _within(got, ref64, atol, rtol):
    got = got.double()
    err = (got - ref64).abs()
    bound = atol + rtol * ref64.abs()
    print(f"max err {float(err.max()):.3e}, max err / bound {float((err / bound).max()):.3f}")
    return bool(torch.isfinite(got).all()) and bool((err <= bound).all())


@pytest.mark.parametrize("gelu", [False, True])
@pytest.mark.parametrize("dim", [64, 256, 96])
def test_layernorm_fp16_output(dev, dim, gelu):
    """dim 64: layernorm64_kernel, 256: the vector path, 96: the scalar path.  With GELU the fp64 bound is that of the LayerNorm
    carried through the GELU (its slope is at most 1.13) plus the 5.5e-5 absolute error of the kernels' erf-GELU approximation
    (csrc/common.h gelu_erf, a documented design choice), which the LayerNorm's own 2e-5 does not cover.  The bit-for-bit comparison with the rounded fp32 output holds in both cases."""
    from micro_sam_amd import ops
    g = torch.Generator().manual_seed(3 + dim)
    rows = 1001
    x = (torch.randn(rows, dim, generator=g) * 3 + 1).to(dev)
    w = torch.randn(dim, generator=g).to(dev)
    b = torch.randn(dim, generator=g).to(dev)
    out16 = ops.layernorm(x, w, b, 1e-6, out_dtype=torch.float16, gelu=gelu)
    out32 = ops.layernorm(x, w, b, 1e-6, out_dtype=torch.float32, gelu=gelu)
    assert out16.dtype == torch.float16 and out16.shape == (rows, dim)
    assert torch.equal(out16, out32.to(torch.float16))
    ref = F.layer_norm(x.double(), (dim,), w.double(), b.double(), eps=1e-6)
    if gelu:
        ref = 0.5 * ref * (1.0 + torch.erf(ref / math.sqrt(2.0)))
        assert _within(out16, ref, 1.13 * 2e-5 + 5.5e-5, 1.13 * 1e-5 + 2.0 ** -11)
    else:
        assert _within(out16, ref, 2e-5, 1e-5 + 2.0 ** -11)


@pytest.mark.parametrize("shape", [(128, 128, 64), (300, 256, 128)])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_gemm_fp16_output(dev, shape, dt):
    """fp16 ``out`` (allocated by the wrapper and handed in) of bf16 and of fp16 operands."""
    from micro_sam_amd import ops
    M, N, K = shape
    g = torch.Generator().manual_seed(7 + M)
    a = torch.randn(M, K, generator=g).to(dt).to(dev)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(dt).to(dev)
    bias = torch.randn(N, generator=g).to(dev)
    out32 = ops.gemm(a, w, bias)
    out16 = ops.gemm(a, w, bias, out_dtype=torch.float16)
    given = torch.empty((M, N), dtype=torch.float16, device=dev)
    assert ops.gemm(a, w, bias, out=given) is given
    assert out16.dtype == torch.float16
    assert torch.equal(out16, out32.to(torch.float16)) and torch.equal(given, out16)
    ref = a.double() @ w.double().t() + bias.double()
    assert _within(out16, ref, 1e-3, 1e-4 + 2.0 ** -11)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_cast_transpose_row_strided(dev, dt):
    """``x[:, :K]`` of a wider buffer and a view with a storage offset: the row stride is handed over, the result is that of the
    contiguous copy bit for bit (the column sums are added in a fixed order)."""
    from micro_sam_amd import ops
    g = torch.Generator().manual_seed(11)
    M, K = 200, 72
    wide = (torch.randn(M + 3, K + 24, generator=g) * 2).to(dt).to(dev)
    for view in (wide[:M, :K], wide[3:, 8:8 + K]):
        assert not view.is_contiguous() and view.stride() == (K + 24, 1)
        got = ops.cast_transpose(view, True, True, True)
        want = ops.cast_transpose(view.contiguous(), True, True, True)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        # against fp64: the casts are one round-to-nearest-even each; M fp32 additions per column are within M * 2^-24 * sum |x|
        ref = view.double()
        assert torch.equal(got[0], view.to(torch.bfloat16)) and torch.equal(got[1], view.to(torch.bfloat16).t())
        assert bool(((got[2].double() - ref.sum(0)).abs() <= M * 2.0 ** -24 * ref.abs().sum(0)).all())


def _table():
    import ops_boundary_table as H
    return H


def _cpu_cases():
    H = _table()
    for entry in H.TABLE:
        for name, path in H.tensor_paths(entry.build()):
            if f"{name}:device" not in entry.skip:
                yield pytest.param(entry, name, path, id=f"{entry.id}-{name}")


@pytest.mark.parametrize("entry,name,path", list(_cpu_cases()))
def test_cpu_tensor_among_device_tensors_is_refused(dev, entry, name, path):
    H = _table()
    kw = entry.build()
    moved = {k: (v.to(dev) if isinstance(v, torch.Tensor) else tuple(e.to(dev) if isinstance(e, torch.Tensor) else e for e in v)
                 if isinstance(v, tuple) and any(isinstance(e, torch.Tensor) for e in v) else v) for k, v in kw.items()}
    moved = H.set_path(moved, path, H.get_path(kw, path))               # this one stays on the host
    with H.recording(real_gpu=True) as rec:
        with pytest.raises((ValueError, TypeError)):
            entry.fn()(**moved)
    assert not rec.calls, f"refused after {rec.names()}"
