"""``ops.semantic_loss`` / ``training.functional.semantic_loss`` (csrc/semloss.hip) on the device, on the cases of
tests/semantic_loss_ref.py: the integer counts exactly; the loss and every entry of the gradient against the fp64 restatement within 4
times the error of the fp32 torch composite (forward and autograd, ON THE DEVICE, in the test itself) against the same fp64 values, with
floors of 2 fp32 ulps of the loss and 2^-22 of the largest gradient entry; bit-identical repeats; the one-pixel form (a view shifted by one
element) against the four-pixel form; the upstream gradient; the refusals.

Measured on an MI355X (over the cases; the test prints every figure, profiles/r08_semantic_loss.md has the table): the kernel's loss
error is 0 to 0.22 of the bound and its gradient error 2.4e-8 to 6.6e-8 of the largest entry, 0.02 to 0.15 of the bound; the device
composite's own loss error is 0 to 1.5e-6 and its gradient error 5.8e-8 to 3.9e-7 of the largest entry."""
import numpy as np
import pytest
import torch

import semantic_loss_ref as R

pytestmark = pytest.mark.gpu
CASES = R.cases()


def _dev(name, shift=False):
    """logits and target of a case on the device; ``shift``: as views one element into larger buffers (4 bytes off 16-byte alignment)."""
    k = CASES[name]
    x, t = torch.as_tensor(k["logits"]), torch.as_tensor(k["target"])
    if not shift:
        return x.cuda(), t.cuda()
    xb = torch.empty(x.numel() + 8, dtype=torch.float32, device="cuda")
    tb = torch.empty(t.numel() + 8, dtype=torch.int32, device="cuda")
    xs, ts = xb[1:1 + x.numel()].view(x.shape), tb[1:1 + t.numel()].view(t.shape)
    xs.copy_(x)
    ts.copy_(t)
    assert xs.is_contiguous() and xs.data_ptr() % 16 == 4 and ts.data_ptr() % 16 == 4
    return xs, ts


def run(name, shift=False, scale=None):
    """Forward and backward through the autograd function -> dict of host values."""
    from micro_sam_amd.training import functional as HF
    k = CASES[name]
    x, t = _dev(name, shift)
    x.requires_grad_()
    loss, stats = HF.semantic_loss(x, t, k["dice_weight"], k["ce_weight"], k["softmax"])
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.is_cuda
    (loss if scale is None else scale * loss).backward()
    assert x.grad.shape == x.shape and x.grad.dtype == torch.float32
    return {"loss": float(loss.detach()), "loss_t": loss.detach().clone(), "raw": stats.raw.clone(), "dice": float(stats.dice), "ce": float(stats.ce),
            "count": stats.count.cpu().numpy(), "n_valid": int(stats.n_valid), "n_ignored": int(stats.n_ignored),
            "ce_sum": float(stats.ce_sum), "num": stats.num.cpu().numpy(), "psq": stats.psq.cpu().numpy(),
            "grad_t": x.grad.detach().clone(), "grad": x.grad.detach().cpu().numpy()}


_YARD = {}


def yardstick(name):
    """The fp32 torch composite on the device (once per case)."""
    if name not in _YARD:
        k = CASES[name]
        _YARD[name] = R.loss_and_gradient(k["logits"], k["target"], torch.float32, k["dice_weight"], k["ce_weight"], k["softmax"], device="cuda")
    return _YARD[name]


def check(name, got, scale=1.0):
    k = CASES[name]
    want, _ = R.reference(name)
    yard = yardstick(name)
    per_class, valid, ignored = R.counts(k["target"], k["logits"].shape[1])
    assert np.array_equal(got["count"], per_class) and got["n_valid"] == valid and got["n_ignored"] == ignored
    bl, bg, yl, yg = R.bounds(want, yard)
    el = abs(got["loss"] - want["loss"])
    eg = float(np.abs(got["grad"].astype(np.float64) - scale * want["grad"]).max())
    gmax = float(np.abs(want["grad"]).max())
    print(f"{name}: loss {want['loss']:.9g} error {el:.3g} = {el / bl:.3f} of the bound (composite {yl:.3g}); gradient error {eg:.3g} = "
          f"{eg / (scale * bg) if bg else 0:.3f} of the bound (composite {yg:.3g} = {yg / gmax if gmax else 0:.3g} of the largest entry)")
    assert np.isfinite(got["loss"]) and np.isfinite(got["grad"]).all()
    assert el <= bl
    assert eg <= scale * bg
    assert abs(got["dice"] - want["dice"]) <= bl and abs(got["ce"] - want["ce"]) <= max(bl, 2 * float(np.spacing(np.float32(abs(want["ce"])))))


@pytest.mark.parametrize("name", sorted(CASES))
def test_loss_and_gradient_equal_the_restatement(name):
    check(name, run(name))


def test_documented_differences_from_torch():
    got = run("33x65_c3_ignored")
    assert got["n_ignored"] == 65 + 3 + 3 + 1 and got["n_valid"] == 2 * 33 * 65 - 72
    got = run("8x8_c3_no_valid")
    assert got["n_valid"] == 0 and got["ce"] == 0.0 and got["ce_sum"] == 0.0 and (got["count"] == 0).all()
    assert got["loss"] == 3.0 and got["dice"] == 3.0 and (got["grad"] == 0).all()
    got = run("16x16_c3_raw_zero_channel")
    assert got["psq"][1] == 0.0 and got["count"][1] == 0 and (got["grad"][:, 1] == 0).all()
    got = run("16x16_c3_pm80")
    assert np.isfinite(got["ce_sum"]) and got["ce"] > 10


def test_one_pixel_and_four_pixel_forms_agree():
    a, b = run("64x64_c3"), run("64x64_c3", shift=True)
    assert np.array_equal(a["count"], b["count"]) and a["n_valid"] == b["n_valid"]
    check("64x64_c3", b)
    want, _ = R.reference("64x64_c3")
    bl, bg, _, _ = R.bounds(want, yardstick("64x64_c3"))
    assert abs(a["loss"] - b["loss"]) <= 2 * bl and np.abs(a["grad"] - b["grad"]).max() <= 2 * bg
    for name in ("12x12_c12_runtime_vec", "192x192_c3_scaled"):
        check(name, run(name, shift=True))


@pytest.mark.parametrize("name", ["192x192_c3_scaled", "513x1024_c2_many_partials", "12x12_c12_runtime_vec", "33x65_c3_ignored"])
def test_two_runs_are_identical(name):
    a, b = run(name), run(name)
    assert torch.equal(a["loss_t"], b["loss_t"]) and torch.equal(a["raw"], b["raw"]) and torch.equal(a["grad_t"], b["grad_t"])


def test_upstream_gradient_is_honoured():
    for name in ("33x65_c3_ignored", "8x8_c9_runtime", "16x16_c3_raw_zero_channel"):
        check(name, run(name, scale=2.5), scale=2.5)
    a, b = run("64x64_c3"), run("64x64_c3", scale=-2.0)
    assert torch.equal(-2.0 * a["grad_t"], b["grad_t"])                  # a power of two: exactly


def test_targets_of_other_types_and_shapes():
    from micro_sam_amd import ops
    x, t = _dev("33x65_c3_ignored")
    base, stats = ops.semantic_loss(x, t)
    for other in (t.long(), t.float(), t[:, None], t[:, None].double(), t.to(torch.int16)):
        loss, s = ops.semantic_loss(x, other)
        assert torch.equal(loss, base) and torch.equal(s.raw, stats.raw)


def test_non_fp32_logits_are_upcast_by_autograd():
    from micro_sam_amd.training import functional as HF
    x, t = _dev("64x64_c3")
    xb = x.to(torch.bfloat16).requires_grad_()
    loss, _ = HF.semantic_loss(xb, t)
    loss.backward()
    xf = xb.detach().float().requires_grad_()
    want, _ = HF.semantic_loss(xf, t)
    want.backward()
    assert torch.equal(loss, want) and xb.grad.dtype == torch.bfloat16 and torch.equal(xb.grad, xf.grad.to(torch.bfloat16))


def test_refusals_leave_the_buffers_untouched():
    from micro_sam_amd import _semloss, ops
    x, t = _dev("33x65_c3_ignored")
    x0, t0 = x.clone(), t.clone()
    _, stats = ops.semantic_loss(x, t)
    raw0 = stats.raw.clone()
    up = torch.ones((), dtype=torch.float32, device="cuda")
    wide = torch.randn(1, 33, 4, 4, device="cuda")
    bad = [
        (ValueError, lambda: ops.semantic_loss(x.cpu(), t)),
        (ValueError, lambda: ops.semantic_loss(x, t.cpu())),
        (ValueError, lambda: ops.semantic_loss(x.transpose(2, 3), t.transpose(1, 2))),
        (ValueError, lambda: ops.semantic_loss(x[:, :, ::2], t[:, ::2])),
        (ValueError, lambda: ops.semantic_loss(x, t.transpose(1, 2).contiguous().transpose(1, 2))),
        (TypeError, lambda: ops.semantic_loss(x.double(), t)),
        (TypeError, lambda: ops.semantic_loss(x.half(), t)),
        (TypeError, lambda: ops.semantic_loss(x, t > 0)),
        (TypeError, lambda: ops.semantic_loss(x.cpu().numpy(), t)),
        (TypeError, lambda: ops.semantic_loss(x, None)),
        (ValueError, lambda: ops.semantic_loss(x, t[:1])),
        (ValueError, lambda: ops.semantic_loss(x, t[:, :, :64])),
        (ValueError, lambda: ops.semantic_loss(x[0], t[0])),
        (ValueError, lambda: ops.semantic_loss(x[:, :1].contiguous(), t)),
        (ValueError, lambda: ops.semantic_loss(wide, torch.zeros(1, 4, 4, dtype=torch.int32, device="cuda"))),
        (ValueError, lambda: ops.semantic_loss(x, t, softmax=False)),
        (ValueError, lambda: ops.semantic_loss(x, t, softmax=False, ce_weight=0.5)),
        (ValueError, lambda: ops.semantic_loss(x, t, dice_weight=float("nan"))),
        (TypeError, lambda: ops.semantic_loss(x, t, ce_weight="1")),
        (TypeError, lambda: ops.semantic_loss_backward(x, t, stats.raw.double(), up)),
        (ValueError, lambda: ops.semantic_loss_backward(x, t, stats.raw[:-1], up)),
        (ValueError, lambda: ops.semantic_loss_backward(x, t, stats, torch.ones(2, device="cuda"))),
        (TypeError, lambda: ops.semantic_loss_backward(x, t, stats, up.double())),
        (ValueError, lambda: ops.semantic_loss_backward(x, t, stats, up.cpu())),
    ]
    for exc, call in bad:
        with pytest.raises(exc):
            call()
    torch.cuda.synchronize()
    assert torch.equal(x, x0) and torch.equal(t, t0) and torch.equal(stats.raw, raw0)
    ok, _ = ops.semantic_loss(x, t, softmax=False, ce_weight=0.0)       # (what the refused combination lacks)
    assert bool(torch.isfinite(ok))
    assert _semloss.SEMLOSS_MAX_CLASSES == 32
