"""Time of the fused semantic-segmentation loss against the torch composite on the device (profiles/r08_semantic_loss.md): forward +
backward of ``training.functional.semantic_loss`` (csrc/semloss.hip: three launches) next to forward + backward of the reference's
formulation with torch operators (tests/semantic_loss_ref.composite: soft-max, one-hot by ``==`` and ``cat``, dice, ``cross_entropy``,
autograd) - what a user of the trainer runs without the kernel - on the same logits and labels, at [2, 3, 512, 512] and [2, 3, 1024, 1024].

Every figure is the median over ``--reps`` windows of ``--inner`` calls each, between two device events, after ``--warmup`` calls of the
same shape; the two forms alternate window by window.  Bytes: what the algorithm needs - forward reads the logits and the labels once,
backward reads them again and writes the gradient: (3 C + 2) * 4 bytes per pixel - over the fused time, against the measured HBM rate of a
float4 copy (MI355X: 6.29 TB/s).  The kernels' own times come from one window under the torch profiler.  Then the error figures of
tests/test_gpu_semantic_loss.py on its cases.  The line "source" names the kernel sources the numbers belong to.

    python tools/semantic_loss_bench.py [--reps 20] [--inner 20] [--warmup 10] [--no-errors]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_MEASURED = 6.29e12                                                  # bytes / s, float4 copy


def _window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner                                    # ms per call


def _kernel_times(fn, inner):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
    each, total = {}, 0.0
    for ev in prof.key_averages():
        t = getattr(ev, "device_time_total", None)
        if t is None:
            t = getattr(ev, "cuda_time_total", 0.0)
        if ev.device_type is not None and str(ev.device_type).endswith("CUDA"):
            total += t / inner
            if "sl_" in ev.key:
                name = ev.key[ev.key.index("sl_"):].split("(")[0]
                each[name] = each.get(name, 0.0) + t / inner
    return {k: v / 1e3 for k, v in each.items()}, total / 1e3           # ms per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-errors", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/semantic_loss_bench.py measures on the device; there is none")
    import bench
    import semantic_loss_ref as R
    from micro_sam_amd.training import functional as HF
    print(json.dumps({"source": bench.csrc_sha16(), "device": torch.cuda.get_device_name(0), "reps": args.reps, "inner": args.inner,
                      "warmup": args.warmup}), flush=True)

    for shape in ((2, 3, 512, 512), (2, 3, 1024, 1024)):
        b, c, h, w = shape
        g = torch.Generator().manual_seed(0)
        x = (2.0 * torch.randn(shape, generator=g)).cuda().requires_grad_()
        t32 = torch.randint(0, c, (b, h, w), generator=g).to(torch.int32).cuda()
        t64 = t32.long()                                                # what cross_entropy takes; the fused call takes int32 as it is

        def fused():
            x.grad = None
            HF.semantic_loss(x, t32)[0].backward()

        def composite():
            x.grad = None
            R.composite(x, t64)[0].backward()
        for fn in (fused, composite):
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        tf, tc = [], []
        for _ in range(args.reps):                                      # alternating: both see the same machine
            tf.append(_window(fused, args.inner))
            tc.append(_window(composite, args.inner))
        fused()
        gf = x.grad.clone()
        composite()
        gc = x.grad.clone()
        nbytes = (3 * c + 2) * 4 * b * h * w
        mf, mc = float(np.median(tf)), float(np.median(tc))
        row = {"shape": list(shape), "fused_ms": mf, "fused_ms_min_max": [min(tf), max(tf)], "composite_ms": mc,
               "composite_ms_min_max": [min(tc), max(tc)], "composite_over_fused": mc / mf, "algorithm_bytes": nbytes,
               "fused_bytes_per_s": nbytes / (mf * 1e-3), "share_of_measured_hbm": nbytes / (mf * 1e-3) / HBM_MEASURED,
               "gradient_max_difference_over_max": float((gf - gc).abs().max() / gc.abs().max())}
        try:
            each, total = _kernel_times(fused, args.inner)
            _, total_c = _kernel_times(composite, args.inner)
            ksum = sum(each.values())
            row.update({"fused_kernels_ms": each, "fused_kernels_ms_sum": ksum, "fused_all_device_ms": total, "composite_all_device_ms": total_c,
                        "kernels_bytes_per_s": nbytes / (ksum * 1e-3) if ksum else None,
                        "kernels_share_of_measured_hbm": nbytes / (ksum * 1e-3) / HBM_MEASURED if ksum else None})
        except Exception as exc:                                        # (profiler unavailable: event times only)
            row["profiler"] = repr(exc)
        print(json.dumps(row), flush=True)

    if args.no_errors:
        return
    for name, k in sorted(R.cases().items()):
        kw = dict(dice_weight=k["dice_weight"], ce_weight=k["ce_weight"], softmax=k["softmax"])
        want, _ = R.reference(name)
        yard = R.loss_and_gradient(k["logits"], k["target"], torch.float32, device="cuda", **kw)
        xs = torch.as_tensor(k["logits"]).cuda().requires_grad_()
        loss, _ = HF.semantic_loss(xs, torch.as_tensor(k["target"]).cuda(), k["dice_weight"], k["ce_weight"], k["softmax"])
        loss.backward()
        bl, bg, yl, yg = R.bounds(want, yard)
        el = abs(float(loss.detach()) - want["loss"])
        eg = float(np.abs(xs.grad.double().cpu().numpy() - want["grad"]).max())
        gmax = float(np.abs(want["grad"]).max()) or 1.0
        print(json.dumps({"case": name, "loss_error": el, "loss_error_over_bound": el / bl, "composite_loss_error": yl,
                          "gradient_error_over_max": eg / gmax, "gradient_error_over_bound": eg / bg if bg else 0.0,
                          "composite_gradient_error_over_max": yg / gmax}), flush=True)


if __name__ == "__main__":
    main()
