"""Time of the volumetric convolutional decoder's 3 x 3 x 3 convolutions and of the whole decoder on the device
(profiles/r10_simple_sam3d.md), forward + backward (dX, dW, db), at B = 1, D = 8 and 1024 x 1024 slices, in two forms run in ONE process:

  (a) ours: ``training.functional.conv3d_k3`` (csrc/conv3d.hip, the implicit GEMM on channels-last rows, fp32 in and out, bf16
      operands) and, for the whole decoder, ``SimpleSam3DWrapper.decode`` (with ``functional.instance_norm_act`` and ``functional.linear``);
  (b) torch in bf16 with ``channels_last_3d`` tensors: ``F.conv3d``, and for the whole decoder ``F.conv3d``, ``F.instance_norm``,
      ``F.leaky_relu`` and ``F.interpolate``.

The five shapes are the first convolution of each of the four blocks and the head's: 256 -> 128 at 64 x 64, 128 -> 64 at 128 x 128,
64 -> 32 at 256 x 256, 32 -> 16 at 512 x 512 and 16 -> 8 at 1024 x 1024 - the same 58 GFLOP per direction each.

Every figure is the median over ``--reps`` windows of at least ``--inner`` calls and at least ``--window-ms`` milliseconds each, between two
device events, after ``--warmup`` calls of both forms (torch's convolution library searches its algorithms in the first call); the forms
alternate window by window (tools/window_timer.py).  Before its timed windows a form runs a few sizing windows, which grow until one is
measured to last ``--window-ms`` (at most 20000 calls; up to profiles/r10_simple_sam3d.md the size came from one 3-call window, capped at 500).  No ratio is fixed in advance: a stage where (a) is slower than (b) is printed as such.  The line "source"
names the kernel sources the numbers belong to.

    python tools/conv3d_bench.py [--reps 7] [--inner 3] [--window-ms 200] [--warmup 3] [--depth 8] [--skip-decoder]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

import window_timer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(64, 256, 128), (128, 128, 64), (256, 64, 32), (512, 32, 16), (1024, 16, 8)]         # (side, Ci, Co)


def compare(forms, args):
    row = window_timer.compare(forms, args)
    if "a" in row and "b" in row:
        row["a_over_b"] = row["a"]["ms"] / row["b"]["ms"]
    return row


def torch_decoder(sd, x):
    """The decoder from torch's operators on channels_last_3d bf16 tensors: x [B, 256, D, 64, 64] -> logits."""
    def conv(t, name, padding):
        return F.conv3d(t, sd[name + ".weight"], sd[name + ".bias"], padding=padding)
    for i in range(4):
        p = f"decoders.{i}."
        residual = F.instance_norm(conv(x, p + "downsample.0", 0))
        out = F.leaky_relu(F.instance_norm(conv(x, p + "conv1.0", 1)), 0.01)
        out = F.instance_norm(conv(out, p + "conv2.0", 1))
        x = F.interpolate(F.leaky_relu(out + residual, 0.01), scale_factor=(1, 2, 2), mode="nearest")
    x = F.leaky_relu(F.instance_norm(conv(x, "out_conv.conv_pred.0", 1)), 0.01)
    return conv(x, "out_conv.segmentation_head", 0)


def main():
    ap = argparse.ArgumentParser()
    window_timer.add_arguments(ap)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--skip-decoder", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/conv3d_bench.py measures on the device; there is none")
    import bench
    from micro_sam_amd.models.simple_sam_3d_wrapper import BasicBlock, SegmentationHead
    from micro_sam_amd.training import functional as HF
    D = args.depth
    print(json.dumps({"source": bench.csrc_sha16(), "device": torch.cuda.get_device_name(0), "reps": args.reps, "inner": args.inner,
                      "window_ms": args.window_ms, "warmup": args.warmup, "depth": D}), flush=True)
    g = torch.Generator().manual_seed(0)
    for side, Ci, Co in SHAPES:
        x = torch.randn(1, D, side, side, Ci, generator=g).cuda().requires_grad_()
        weight = torch.nn.Parameter((torch.randn(Co, Ci, 3, 3, 3, generator=g) * (27 * Ci) ** -0.5).cuda())
        bias = torch.nn.Parameter(torch.randn(Co, generator=g).cuda())
        dy = torch.randn(1, D, side, side, Co, generator=g).cuda()
        x16 = x.detach().permute(0, 4, 1, 2, 3).to(torch.bfloat16).contiguous(memory_format=torch.channels_last_3d).requires_grad_()
        w16 = torch.nn.Parameter(weight.detach().to(torch.bfloat16).contiguous(memory_format=torch.channels_last_3d))
        b16 = torch.nn.Parameter(bias.detach().to(torch.bfloat16))
        dy16 = dy.permute(0, 4, 1, 2, 3).to(torch.bfloat16).contiguous(memory_format=torch.channels_last_3d)
        kept = {}

        def form_a():
            for t in (x, weight, bias):
                t.grad = None
            out = HF.conv3d_k3(x, weight, bias)
            out.backward(dy)
            kept["a"] = (out.detach(), x.grad, weight.grad)

        def form_b():
            for t in (x16, w16, b16):
                t.grad = None
            out = F.conv3d(x16, w16, b16, padding=1)
            out.backward(dy16)
            kept["b"] = (out.detach().permute(0, 2, 3, 4, 1).float(), x16.grad.permute(0, 2, 3, 4, 1).float(), w16.grad.float())

        row = compare({"a": form_a, "b": form_b}, args)
        flops = 2.0 * D * side * side * 27 * Ci * Co * 3                # forward, dX, dW
        row.update(shape={"side": side, "Ci": Ci, "Co": Co, "M": D * side * side}, flops_forward_backward=flops)
        for k in ("a", "b"):
            if k in row:
                row[k]["flops_per_s"] = flops / (row[k]["ms"] * 1e-3)
        if "a" in kept and "b" in kept:
            row["difference_b_from_a_over_max"] = [float((p - q).abs().max() / q.abs().max()) for p, q in zip(kept["b"], kept["a"])]
        print(json.dumps(row), flush=True)
        del x, x16, dy, dy16, kept
        torch.cuda.empty_cache()
    if args.skip_decoder:
        return
    torch.manual_seed(0)
    model = torch.nn.Module()
    model.decoders = torch.nn.ModuleList([BasicBlock(256, 128), BasicBlock(128, 64), BasicBlock(64, 32), BasicBlock(32, 16)])
    model.out_conv = SegmentationHead(16, args.classes)
    model.cuda()
    feats = torch.randn(1, D, 64, 64, 256, generator=g).cuda()
    gout = torch.randn(1, D, 1024, 1024, args.classes, generator=g).cuda()
    sd16 = {k: v.detach().to(torch.bfloat16).contiguous(memory_format=torch.channels_last_3d if v.dim() == 5 else torch.contiguous_format)
            .requires_grad_() for k, v in model.state_dict().items()}
    feats16 = feats.permute(0, 4, 1, 2, 3).to(torch.bfloat16).contiguous(memory_format=torch.channels_last_3d)
    gout16 = gout.permute(0, 4, 1, 2, 3).to(torch.bfloat16).contiguous(memory_format=torch.channels_last_3d)

    def decoder_a():
        model.zero_grad(set_to_none=True)
        out = feats
        for block in model.decoders:
            out = block(out)
        model.out_conv(out).backward(gout)

    def decoder_b():
        for v in sd16.values():
            v.grad = None
        torch_decoder(sd16, feats16).backward(gout16)

    row = compare({"a": decoder_a, "b": decoder_b}, args)
    row["decoder"] = {"depth": D, "classes": args.classes}
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
