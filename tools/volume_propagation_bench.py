"""Timing of ``multi_dimensional_segmentation.segment_objects_in_volume`` on the device (profiles/r11_volume_propagation.md): one volume
of 16 slices of 512 x 512 (``synthetic_tile``), about 20 disks seeded in their middle slices, vit_b with the synthetic weights,
projection "mask", embeddings computed once and kept on the device.  The batched device path against the per-object loop it replaces
(``_objects_per_object_loop``: N calls of ``segment_mask_in_volume``) on the same embeddings: wall time of a whole call, median of
--reps runs after one warm-up each.  Also reported: in how many pixels and ranges the two results differ (they can differ only through
the decoder's batching and the handful of mask-prompt pixels within rounding of 0.5), and the same for ``batch_size=1``.

    python tools/volume_propagation_bench.py [--reps 5] [--slices 16] [--size 512] [--objects 20] [--projection mask]
    python tools/volume_propagation_bench.py --once          # one warm-up + one device-path call (for a kernel trace)
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _seeds(n, size, slices, rng):
    yy, xx = np.mgrid[0:size, 0:size]
    seeds, zs = [], []
    for _ in range(n):
        cy, cx, r = rng.uniform(0.1 * size, 0.9 * size), rng.uniform(0.1 * size, 0.9 * size), rng.uniform(0.03 * size, 0.12 * size)
        seeds.append(((yy - cy) ** 2 + (xx - cx) ** 2 < r * r).astype(np.uint8))
        zs.append(int(rng.integers(slices // 4, 3 * slices // 4)))
    return np.stack(seeds), np.array(zs)


def _wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slices", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--objects", type=int, default=20)
    ap.add_argument("--projection", default="mask")
    ap.add_argument("--iou-threshold", type=float, default=1e-6)      # the synthetic weights give small IoUs: (almost) nothing stops
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    from micro_sam_amd import multi_dimensional_segmentation as M
    from micro_sam_amd import util
    from micro_sam_amd.synthetic import synthetic_state_dict, synthetic_tile
    sha = hashlib.sha256(open(os.path.join(ROOT, "micro_sam_amd", "csrc", "propagate.hip"), "rb").read()).hexdigest()[:16]
    predictor = util.get_sam_model("vit_b", device="cuda", state_dict=synthetic_state_dict("vit_b", 0))
    volume = np.stack([synthetic_tile(100 + z, (args.size, args.size)) for z in range(args.slices)])
    emb = util.precompute_image_embeddings(predictor, volume, ndim=3, verbose=False)
    seeds, zs = _seeds(args.objects, args.size, args.slices, np.random.default_rng(3))
    ids = np.arange(1, args.objects + 1)
    common = dict(iou_threshold=args.iou_threshold, projection=args.projection, box_extension=0.025)

    def device(batch_size=64):
        return M.segment_objects_in_volume(predictor, emb, seeds, zs, ids, batch_size=batch_size, **common)

    def loop():
        return M._objects_per_object_loop(predictor, emb, seeds, zs, ids, common["iou_threshold"], common["projection"],
                                          common["box_extension"], False)
    if args.once:
        device()
        torch.cuda.synchronize()
        device()
        torch.cuda.synchronize()
        return
    got, ranges = device()
    one, ranges_one = device(batch_size=1)
    want, want_ranges = loop()

    def decoded(r):              # (object, slice) decodes: the accepted steps and the one that stopped a walk before the volume's end
        return int((r[:, 1] - r[:, 0]).sum() + (r[:, 1] < args.slices - 1).sum() + (r[:, 0] > 0).sum())
    print(json.dumps({"propagate_hip_sha256_16": sha, "device": torch.cuda.get_device_name(0), "slices": args.slices, "size": args.size,
                      "objects": args.objects, **common, "accepted_steps_device": int((ranges[:, 1] - ranges[:, 0]).sum()),
                      "accepted_steps_loop": int((want_ranges[:, 1] - want_ranges[:, 0]).sum()), "decoded_steps_device": decoded(ranges),
                      "decoded_steps_loop": decoded(want_ranges),
                      "pixels_differ_batched_vs_loop": int((got != want).sum()), "ranges_differ_batched_vs_loop": int((ranges != want_ranges).sum()),
                      "pixels_differ_batch1_vs_loop": int((one != want).sum()), "ranges_differ_batch1_vs_loop": int((ranges_one != want_ranges).sum()),
                      "pixels_differ_batched_vs_batch1": int((got != one).sum()), "labelled_pixels": int((want != 0).sum())}), flush=True)
    for name, fn in (("segment_objects_in_volume (device path, batch 64)", device), ("per-object loop (segment_mask_in_volume x N)", loop)):
        s = _wall(fn, args.reps)
        print(json.dumps({"variant": name, "s_median": float(np.median(s)), "s_min": float(np.min(s)), "s_max": float(np.max(s)),
                          "reps": args.reps}), flush=True)


if __name__ == "__main__":
    main()
