"""Timing of the prompt derivation of the AutomaticPromptGenerator (profiles/apg_prompt_derivation.md): the host function
``instance_segmentation._derive_point_prompts`` on maps that are already on the host next to ``_derive_point_prompts_device``
(``ops.seed_centers``, csrc/labelprops.hip) on maps that are already on the device, the copy of the points to the host included.  Same
process, the two routes alternating, a host clock around each call; every device call is followed by a synchronise.  Two seeded
1024 x 1024 inputs: the 24 disks of tests/test_gpu_prompt_generator.py with their ideal decoder maps, and a dense one - 400 disks of radius 6..17
painted one over the other, with the ideal decoder maps of that label image.  Then ``AutomaticPromptGenerator.generate()`` end to end on the dense
input, once with the decoder output kept on the device and once from a restored state (the host route).

    python tools/apg_prompt_derivation_bench.py [--reps 20] [--no-generate]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def dense_labels(shape=(1024, 1024), n=400, seed=0):
    """400 disks of radius 6..17 painted one over the other (a later disk overwrites an earlier one)."""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    out = np.zeros(shape, np.uint32)
    for k in range(n):
        cy, cx, r = g.integers(0, shape[0]), g.integers(0, shape[1]), g.integers(6, 18)
        out[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = k + 1
    return out


def ideal_maps(labels):
    """Ideal decoder maps in the manner of oracle/apg_ref.decoder_maps_from_labels, computed per zero-padded bounding box instead of with
    one full-image transform per object (so the image border counts as a boundary).  An input generator, nothing more."""
    from scipy import ndimage as ndi
    fg = (labels > 0).astype("float32")
    center = np.ones(labels.shape, dtype="float32")
    boundary = np.ones(labels.shape, dtype="float32")
    for idx, bb in enumerate(ndi.find_objects(labels.astype(np.int64))):
        if bb is None:
            continue
        m = np.pad(labels[bb] == idx + 1, 1)
        d = ndi.distance_transform_edt(m)
        cy, cx = np.unravel_index(np.argmax(d), d.shape)
        yy, xx = np.nonzero(m)
        dc = np.sqrt((yy - cy) ** 2 + (xx - cx) ** 2)
        inner = (slice(1, -1), slice(1, -1))
        b, c = np.ones(m.shape, "float32"), np.ones(m.shape, "float32")
        b[m] = 1.0 - (d[m] / d.max())
        c[m] = dc / max(dc.max(), 1e-6)
        boundary[bb][m[inner]] = b[inner][m[inner]]
        center[bb][m[inner]] = c[inner][m[inner]]
    return fg, center, boundary


def _stats(ms):
    return {"ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_p90": float(np.percentile(ms, 90)), "ms_max": float(np.max(ms)),
            "reps": len(ms)}


def _alternate(host_fn, device_fn, reps):
    """[host ms], [device ms]: one warm-up of each, then host, device, host, device, ..."""
    host_fn()
    device_fn()
    torch.cuda.synchronize()
    host, dev = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        host_fn()
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        device_fn()
        torch.cuda.synchronize()
        dev.append((time.perf_counter() - t0) * 1e3)
    return host, dev


def _kernel_times(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    rows = {}
    for ev in prof.key_averages():
        t = getattr(ev, "device_time_total", None)
        if t is None:
            t = getattr(ev, "cuda_time_total", 0.0)
        if ev.device_type is not None and str(ev.device_type).endswith("CUDA") and t > 0:
            rows[ev.key[:60]] = round(t / 1e3, 4)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-generate", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: nothing here is measured without one")
    from micro_sam_amd import instance_segmentation as IS
    from oracle import apg_ref as G
    from test_gpu_prompt_generator import _disk_labels
    sha = hashlib.sha256(open(os.path.join(ROOT, "micro_sam_amd", "csrc", "labelprops.hip"), "rb").read()).hexdigest()[:16]
    inputs = {"24 disks": G.decoder_maps_from_labels(_disk_labels((1024, 1024), 24, seed=1)), "dense": ideal_maps(dense_labels())}
    print(json.dumps({"labelprops_hip_sha256_16": sha, "device": torch.cuda.get_device_name(0), "reps": args.reps}), flush=True)
    for name, maps in inputs.items():
        dev_maps = [torch.from_numpy(np.ascontiguousarray(m)).cuda() for m in maps]
        want, got = IS._derive_point_prompts(*maps), IS._derive_point_prompts_device(*dev_maps)
        same = np.array_equal(want["points"], got["points"]) and np.array_equal(want["point_labels"], got["point_labels"])
        host, dev = _alternate(lambda: IS._derive_point_prompts(*maps), lambda: IS._derive_point_prompts_device(*dev_maps), args.reps)
        print(json.dumps({"input": name, "components": int(len(want["points"])), "device_equals_host": bool(same),
                          "host _derive_point_prompts": _stats(host), "device _derive_point_prompts_device": _stats(dev)}), flush=True)
        try:
            print(json.dumps({"kernels_ms_of_one_device_call": name, **_kernel_times(lambda: IS._derive_point_prompts_device(*dev_maps))}), flush=True)
        except Exception as exc:          # (profiler unavailable: call times only)
            print("profiler:", exc, flush=True)
    if args.no_generate:
        return
    from micro_sam_amd import util
    from micro_sam_amd.synthetic import synthetic_state_dict, synthetic_tile
    predictor = util.get_sam_model("vit_b", device="cuda", state_dict=synthetic_state_dict("vit_b", 0))
    tile = synthetic_tile(7)
    emb = util.precompute_image_embeddings(predictor, tile, verbose=False)
    stacked = torch.from_numpy(np.stack(inputs["dense"]))[None].cuda()
    on_device = IS.AutomaticPromptGenerator(predictor, lambda *a: stacked)
    on_device.initialize(tile, image_embeddings=emb)
    restored = IS.AutomaticPromptGenerator(predictor, None)
    restored.set_state(on_device.get_state())
    routed = getattr(on_device, "_device_maps", None) is not None
    a, b = restored.generate(), on_device.generate()
    host, dev = _alternate(restored.generate, on_device.generate, args.reps)
    print(json.dumps({"generate() on": "dense", "device_route_taken": bool(routed), "objects": int(a.max()), "same_image": bool(np.array_equal(a, b)),
                      "host route (restored state)": _stats(host), "device route (decoder output on the device)": _stats(dev)}), flush=True)


if __name__ == "__main__":
    main()
