"""Fine-tuning's fp32 attention kernels on the device (csrc/train.hip: ``attn_fwd`` / ``attn_bwd_q`` / ``attn_bwd_kv`` thread-per-row and
``_rowblock``, ``relpos_fwd`` / ``relpos_bwd_q`` / ``relpos_bwd_kv``) through the raw ABI (``msam_attention_forward`` / ``_backward``,
``msam_relpos_attention_forward`` / ``_backward``), so that ``lse`` and ``delta`` - outputs the backward pass consumes - are seen.

Reference, bounds, input families and the case table are tests/train_attention_ref.py (read its docstring first): exact cases where the
arithmetic allows (``uniform``: the mean bit for bit; ``onehot``: a bit-exact gather / scatter, also of non-zero gradients through the
shifted backward call), per-element float64 rounding bounds elsewhere (``diffuse``, ``peaked`` in three key orders, and the exact
families too).  The shapes are the smallest that reach each branch: both sides of the row-block route conditions, short last strides,
block edges, Gw at the LDS limit with a partial block, Gh > 64.  tests/test_train_attention_host.py runs the same table on the CPU and
shows by mutation that the exact assertions notice a wrong kernel.

Every output is a slice of a larger buffer between two guard zones of a fixed bit pattern that must come back unchanged (a write past
a row is seen without provoking anything), is pre-filled with NaN (an element that is not written is seen), and every call is repeated
once and must return the same bits (no atomics).  The workload-sized shapes stay in tests/test_gpu_training.py and
tests/test_gpu_training_encoders.py."""
import math

import numpy as np
import pytest
import torch

import train_attention_ref as R

pytestmark = pytest.mark.gpu

GUARD = 256                        # floats before and after every output
PATTERN = 0x7FA5C3E1               # a NaN


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


class DeviceBackend:
    """The raw ABI on device tensors; outputs between guard zones."""

    def __init__(self, dev):
        from micro_sam_amd import _lib
        self.dev, self._lib, self.lib = dev, _lib, _lib.load()

    def _out(self, shape):
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * GUARD,), PATTERN, dtype=torch.int32, device=self.dev)
        return buf, buf[GUARD:GUARD + n].view(torch.float32).view(shape)

    def _dev(self, *arrays):
        return [torch.from_numpy(np.ascontiguousarray(a)).to(self.dev) for a in arrays]

    def _finish(self, what, bufs):
        res = []
        for buf, view in bufs:
            assert bool((buf[:GUARD] == PATTERN).all()) and bool((buf[-GUARD:] == PATTERN).all()), f"{what}: a guard zone was written"
            res.append(view.cpu().numpy().copy())
        return res

    def forward(self, c):
        bufs = [self._out((c.BH, c.Nq, c.D)), self._out((c.BH, c.Nq))]
        o, l = (v.data_ptr() for _, v in bufs)
        if c.op == "plain":
            q, k, v = self._dev(c.q, c.k, c.v)
            self._lib.check(self.lib.msam_attention_forward(q.data_ptr(), k.data_ptr(), v.data_ptr(), c.BH, c.Nq, c.Nk, c.D, float(c.scale), o, l,
                                                            self._lib.stream_ptr()), "msam_attention_forward")
        else:
            q, k, v, bh, bw = self._dev(c.q, c.k, c.v, c.bias_h, c.bias_w)
            self._lib.check(self.lib.msam_relpos_attention_forward(q.data_ptr(), k.data_ptr(), v.data_ptr(), bh.data_ptr(), bw.data_ptr(), c.BH, c.Gh,
                                                                   c.Gw, c.D, float(c.scale), o, l, self._lib.stream_ptr()),
                            "msam_relpos_attention_forward")
        return self._finish("forward", bufs)

    def backward(self, c, out, lse):
        qs, ks = (c.BH, c.Nq, c.D), (c.BH, c.Nk, c.D)
        if c.op == "plain":
            names = ("dq", "dk", "dv", "delta")
            bufs = [self._out(s) for s in (qs, ks, ks, (c.BH, c.Nq))]
            q, k, v, o, do, l = self._dev(c.q, c.k, c.v, out, c.dout, lse)
            self._lib.check(self.lib.msam_attention_backward(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), l.data_ptr(), c.BH,
                                                             c.Nq, c.Nk, c.D, float(c.scale), *[v_.data_ptr() for _, v_ in bufs],
                                                             self._lib.stream_ptr()), "msam_attention_backward")
        else:
            names = ("dq", "dk", "dv", "dbias_h", "dbias_w", "delta")
            bufs = [self._out(s) for s in (qs, ks, ks, (c.BH, c.Nq, c.Gh), (c.BH, c.Nq, c.Gw), (c.BH, c.Nq))]
            q, k, v, bh, bw, o, do, l = self._dev(c.q, c.k, c.v, c.bias_h, c.bias_w, out, c.dout, lse)
            self._lib.check(self.lib.msam_relpos_attention_backward(q.data_ptr(), k.data_ptr(), v.data_ptr(), bh.data_ptr(), bw.data_ptr(), o.data_ptr(),
                                                                    do.data_ptr(), l.data_ptr(), c.BH, c.Gh, c.Gw, c.D, float(c.scale),
                                                                    *[v_.data_ptr() for _, v_ in bufs], self._lib.stream_ptr()),
                            "msam_relpos_attention_backward")
        return dict(zip(names, self._finish("backward", bufs)))


@pytest.fixture(scope="module")
def gpu(dev):
    return DeviceBackend(dev)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nlargest err / bound on the device:\n" + R.format_ratios("gpu"))


def _run_shape(gpu, op, shape, D):
    fails = []
    for case in R.case_list(op):
        if case[1] != shape or case[2] != D:
            continue
        c = R.make_case(*case)
        got = R.run_case(gpu, c)
        fails += R.check_case(c, got, "gpu")
        again = R.run_case(gpu, c)                                         # no atomics: the same bits on every call
        for n in got:
            if not np.array_equal(got[n].view(np.uint32), again[n].view(np.uint32)):
                fails.append(("exact", n, f"{op} {shape} D={D} {c.family}: {n}: the second call returned other bits"))
    assert not fails, "\n".join(f[2] for f in fails)


@pytest.mark.parametrize("D", R.PLAIN_DIMS)
@pytest.mark.parametrize("shape", R.PLAIN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_plain_attention_exact_cases_and_fp64_bounds(gpu, shape, D):
    """(Nq, Nk): every family of the table - uniform, one-hot (all variants), diffuse, peaked in three key orders."""
    _run_shape(gpu, "plain", shape, D)


@pytest.mark.parametrize("D", R.RELPOS_DIMS)
@pytest.mark.parametrize("shape", R.RELPOS_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_relpos_attention_exact_cases_and_fp64_bounds(gpu, shape, D):
    """(Gh, Gw): every family of the table."""
    _run_shape(gpu, "relpos", shape, D)


def test_intrinsics_are_within_the_constant_the_bounds_use(gpu):
    """E_INTRINSIC measured where a float64 value isolates the intrinsic.  __expf: two keys with logits (0, -x), v = (e_0, e_1), so that
    out = (1, p) / (1 + p) with p = exp(-x); apart from the exponential only 1 + p, the reciprocal and the product round (3 u).  __logf:
    the uniform family, lse = log Nk with l = Nk exact.  Prints the measured constants in units of u."""
    D, n = 16, 321
    x = 0.25 * np.arange(n)                                               # 0 .. 80; -x = (x / 4) * (-4) is exact on every path
    c = R.make_case("plain", (n, 2), D, "diffuse")
    c.q[...] = 0
    c.q[:, :, 0] = x
    c.k[...] = 0
    c.k[:, 1, 0] = -4
    c.v[...] = 0
    c.v[:, 0, 0] = c.v[:, 1, 1] = 1
    out, _ = gpu.forward(c)
    p = np.exp(-x)
    ref = p / (1 + p)
    rel = np.abs(out[:, :, 1].astype(np.float64) - ref) / ref
    e_exp = float(((rel - 3 * R.U) / ((1 + x) * R.U)).max())
    assert np.abs(out[:, :, 0].astype(np.float64) - 1 / (1 + p)).max() <= 2 * 4 * R.U
    e_log = 0.0
    for nk in (2, 3, 5, 7, 10, 100, 130, 1000, 1025, 1279):
        u = R.make_case("plain", (1, nk), D, "uniform")
        _, lse = gpu.forward(u)
        e_log = max(e_log, float(np.abs(lse.astype(np.float64) - math.log(nk)).max() / (R.U * math.log(nk))))
    print(f"\nmeasured on the device, in units of u: __expf E = {e_exp:.3f} (bounds use {R.E_INTRINSIC}), "
          f"__logf {e_log:.3f} (bounds use {R.E_INTRINSIC + 1}: the instruction and the product with ln 2)")
    assert e_exp <= R.E_INTRINSIC and e_log <= R.E_INTRINSIC + 1


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def test_autograd_wrappers_on_transposed_views_give_the_raw_call_bits(gpu, dev):
    """HF.attention / HF.relpos_attention on non-contiguous head-transposed views ([B, N, H, D].transpose(1, 2), as the model calls them)
    against the raw ABI on contiguous copies: the same bits for the output and every gradient."""
    from micro_sam_amd.training import functional as HF
    c = R.make_case("plain", (3, 1025), 32, "diffuse")                     # the row-block route
    base = [torch.from_numpy(a.reshape(1, R.BH, -1, c.D)).to(dev).transpose(1, 2).contiguous().requires_grad_() for a in (c.q, c.k, c.v)]
    q, k, v = (b.transpose(1, 2) for b in base)                            # [B, H, N, D] views of [B, N, H, D] storage
    assert not q.is_contiguous() and not k.is_contiguous()
    out = HF.attention(q, k, v)
    do = torch.from_numpy(c.dout.reshape(1, R.BH, c.Nq, c.D)).to(dev)
    out.backward(do.transpose(1, 2).contiguous().transpose(1, 2))
    raw = R.run_case(gpu, c)
    assert np.array_equal(_bits(out).cpu().numpy().reshape(-1), raw["out"].view(np.int32).reshape(-1))
    for b, n in zip(base, ("dq", "dk", "dv")):
        assert np.array_equal(_bits(b.grad.transpose(1, 2)).cpu().numpy().reshape(-1), raw[n].view(np.int32).reshape(-1)), n
    c = R.make_case("relpos", (3, 64), 80, "diffuse")                      # the LDS limit with a partial block
    base = [torch.from_numpy(a).to(dev).transpose(0, 1).contiguous().requires_grad_() for a in (c.q, c.k, c.v, c.bias_h, c.bias_w)]
    ins = [b.transpose(0, 1) for b in base]                                # [BH, N, .] views of [N, BH, .] storage
    assert not ins[0].is_contiguous()
    out = HF.relpos_attention(*ins, float(c.scale))
    out.backward(torch.from_numpy(c.dout).to(dev))
    raw = R.run_case(gpu, c)
    assert np.array_equal(_bits(out).cpu().numpy().reshape(-1), raw["out"].view(np.int32).reshape(-1))
    for b, n in zip(base, ("dq", "dk", "dv", "dbias_h", "dbias_w")):
        assert np.array_equal(_bits(b.grad.transpose(0, 1)).cpu().numpy().reshape(-1), raw[n].view(np.int32).reshape(-1)), n


def test_refusals_raise_and_leave_the_outputs_alone(gpu, dev):
    """Gw = 65 (over the kernel's LDS column array) raises through the wrapper and the raw calls leave pre-filled outputs untouched;
    D = 24 raises for plain attention, D = 32 for rel-pos."""
    from micro_sam_amd import _lib
    from micro_sam_amd.training import functional as HF
    z = lambda *s: torch.zeros(s, device=dev)
    with pytest.raises(ValueError):
        HF.relpos_attention(z(1, 65, 64), z(1, 65, 64), z(1, 65, 64), z(1, 65, 1), z(1, 65, 65), 0.125)
    with pytest.raises(ValueError):
        HF.attention(z(1, 1, 4, 24), z(1, 1, 4, 24), z(1, 1, 4, 24))
    with pytest.raises(ValueError):
        HF.relpos_attention(z(1, 4, 32), z(1, 4, 32), z(1, 4, 32), z(1, 4, 2), z(1, 4, 2), 0.125)
    lib, sp = gpu.lib, _lib.stream_ptr()
    i65, b1, b65, r65 = z(1, 65, 64), z(1, 65, 1), z(1, 65, 65), z(1, 65)
    bufs = [gpu._out(s) for s in ((1, 65, 64), (1, 65))]
    assert lib.msam_relpos_attention_forward(i65.data_ptr(), i65.data_ptr(), i65.data_ptr(), b1.data_ptr(), b65.data_ptr(), 1, 1, 65, 64, 0.125,
                                             *[v.data_ptr() for _, v in bufs], sp) == 1
    bufs += [gpu._out(s) for s in ((1, 65, 64), (1, 65, 64), (1, 65, 64), (1, 65, 1), (1, 65, 65), (1, 65))]
    assert lib.msam_relpos_attention_backward(i65.data_ptr(), i65.data_ptr(), i65.data_ptr(), b1.data_ptr(), b65.data_ptr(), i65.data_ptr(),
                                              i65.data_ptr(), r65.data_ptr(), 1, 1, 65, 64, 0.125, *[v.data_ptr() for _, v in bufs[2:]], sp) == 1
    i24, r4 = z(1, 4, 24), z(1, 4)
    bufs += [gpu._out(s) for s in ((1, 4, 24), (1, 4))]
    assert lib.msam_attention_forward(i24.data_ptr(), i24.data_ptr(), i24.data_ptr(), 1, 4, 4, 24, 0.2, *[v.data_ptr() for _, v in bufs[8:]], sp) == 1
    bufs += [gpu._out(s) for s in ((1, 4, 24), (1, 4, 24), (1, 4, 24), (1, 4))]
    assert lib.msam_attention_backward(i24.data_ptr(), i24.data_ptr(), i24.data_ptr(), i24.data_ptr(), i24.data_ptr(), r4.data_ptr(), 1, 4, 4, 24, 0.2,
                                       *[v.data_ptr() for _, v in bufs[10:]], sp) == 1
    i32, b2 = z(1, 4, 32), z(1, 4, 2)
    bufs += [gpu._out(s) for s in ((1, 4, 32), (1, 4))]
    assert lib.msam_relpos_attention_forward(i32.data_ptr(), i32.data_ptr(), i32.data_ptr(), b2.data_ptr(), b2.data_ptr(), 1, 2, 2, 32, 0.125,
                                             *[v.data_ptr() for _, v in bufs[14:]], sp) == 1
    torch.cuda.synchronize()
    assert all(bool((b == PATTERN).all()) for b, _ in bufs)
