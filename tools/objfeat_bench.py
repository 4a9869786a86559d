"""Timing of object_classification.compute_object_features on the device (profiles/r07_object_features.md): per case the wall time of a
call (inputs already on the device, synchronised), the device time of the objfeat kernels and of all kernels of the call (torch profiler),
per call and per unit, next to the CPU restatement of the reference (tests/object_features_ref.py) on the same input.

    python tools/objfeat_bench.py [--reps 5] [--no-cpu]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _device_times(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    total = objfeat = 0.0
    for ev in prof.key_averages():
        t = getattr(ev, "device_time_total", None)
        if t is None:
            t = getattr(ev, "cuda_time_total", 0.0)
        if ev.device_type is not None and str(ev.device_type).endswith("CUDA"):
            total += t
            if "objfeat" in ev.key:
                objfeat += t
    return objfeat / 1e3, total / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    from micro_sam_amd import object_classification as OC
    from micro_sam_amd import util
    from micro_sam_amd.synthetic import synthetic_state_dict, synthetic_tile_with_labels
    import object_features_ref as REF
    predictor = util.get_sam_model("vit_b", device="cuda:0", state_dict=synthetic_state_dict("vit_b", 0))
    image, labels = synthetic_tile_with_labels(1, (1024, 1024))
    pairs = [synthetic_tile_with_labels(20 + z, (1024, 1024)) for z in range(4)]
    vol, vlab = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    cases = []
    e2 = util.precompute_image_embeddings(predictor, image, verbose=False, keep_on_device=True)
    cases.append(("2d 1024x1024", e2, labels, 1, lambda: REF.compute_object_features(e2["features"].cpu().numpy(), labels)))
    et = util.precompute_image_embeddings(predictor, image, tile_shape=(512, 512), halo=(64, 64), verbose=False)
    from test_gpu_object_classification import _HostTiles, _blocks
    n_tiles = len(et["features"])
    cases.append(("2d tiled 512 / halo 64", et, labels, n_tiles,
                  lambda: REF.compute_object_features(_HostTiles(et["features"]), labels, is_tiled=True, tile_blocks=_blocks(et["features"]))))
    e3 = util.precompute_image_embeddings(predictor, vol, verbose=False, keep_on_device=True)
    cases.append(("3d 4 x 1024x1024", e3, vlab, 4, lambda: REF.compute_object_features(e3["features"].cpu().numpy(), vlab)))
    out = []
    for name, emb, lab, units, cpu in cases:
        lab_dev = torch.from_numpy(lab).cuda()
        OC.compute_object_features(emb, lab_dev, verbose=False)
        torch.cuda.synchronize()
        walls = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            OC.compute_object_features(emb, lab_dev, verbose=False)
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
        try:
            k_obj, k_all = _device_times(lambda: OC.compute_object_features(emb, lab_dev, verbose=False))
        except Exception as exc:          # (profiler unavailable: wall times only)
            print("profiler:", exc)
            k_obj = k_all = float("nan")
        row = {"case": name, "units": units, "objects": int(len(np.unique(lab)) - 1), "wall_ms_median": float(np.median(walls)),
               "objfeat_kernels_ms": k_obj, "all_kernels_ms": k_all, "objfeat_kernels_ms_per_unit": k_obj / units}
        if not args.no_cpu:
            t0 = time.perf_counter()
            cpu()
            row["cpu_restatement_s"] = time.perf_counter() - t0
        out.append(row)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
