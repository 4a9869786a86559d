"""The merge stage of automatic_3d_segmentation on a GPU: the device route (csrc/merge3d.hip) against the host route, which is the
route of the commit before the device merge (profiles/merge3d_device.md).

    python tools/merge3d_bench.py [--slices 64] [--host-reps 1] [--out FILE]      both routes on a seeded volume, one JSON record
    python tools/merge3d_bench.py --trace                                           msam_close_gaps alone, six calls, for a kernel trace
                                                                                    (rocprofv3 --kernel-trace --stats -- python ...)

The volume: one ``synthetic_tile`` (1024 x 1024) with fresh noise per slice, so that the objects run through z, and one blank slice;
"cells" weights, the default generator with both thresholds at 0.5 (a few hundred objects per slice).  Host clocks around steps that
end in a device synchronise; the closing alone with device events.  The two routes must give the same volume (``routes_equal``)."""
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
SOURCES = ("micro_sam_amd/csrc/merge3d.hip", "micro_sam_amd/_merge3d.py", "micro_sam_amd/multi_dimensional_segmentation.py",
           "include/msam_hip.h")


def source_hash() -> str:
    h = hashlib.sha1()
    for f in SOURCES:
        h.update(open(os.path.join(ROOT, f), "rb").read())
    return h.hexdigest()[:16]


def trace():
    """64 x 1024 x 1024, 441 discs per slice with running ids, one blank slice, gap 1."""
    from micro_sam_amd import ops
    Z = 64
    yy, xx = np.ogrid[:1024, :1024]
    sl = np.zeros((1024, 1024), np.int32)
    k = 0
    for cy in range(24, 1024, 48):
        for cx in range(24, 1024, 48):
            k += 1
            sl[(yy - cy) ** 2 + (xx - cx) ** 2 <= 18 * 18] = k
    vol = np.stack([np.where(sl > 0, sl + z * k, 0) for z in range(Z)]).astype(np.int32)
    vol[Z // 2] = 0
    t = torch.as_tensor(vol).cuda()
    for _ in range(6):
        _, result = ops.close_gaps_z(t, 1, id_limit=int(vol.max()) + 1)
    torch.cuda.synchronize()
    print("discs per slice", k, "result", result.tolist(), "source", source_hash())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", type=int, default=64)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("merge3d_bench: needs a GPU")
    if args.trace:
        return trace()
    from micro_sam_amd import multi_dimensional_segmentation as M
    from micro_sam_amd import ops, util
    from micro_sam_amd.instance_segmentation import AutomaticMaskGenerator
    from micro_sam_amd.synthetic import synthetic_state_dict, synthetic_tile
    Z = args.slices
    rep = {"source_sha1": source_hash(), "Z": Z, "device": torch.cuda.get_device_name(0)}
    dev = torch.device("cuda", 0)
    predictor = util.get_sam_model("vit_b", device=dev, state_dict=synthetic_state_dict("vit_b", 0, variant="cells"))
    base = synthetic_tile(3, (1024, 1024)).astype(np.float32)
    rng = np.random.default_rng(0)
    vol = np.stack([np.clip(base + rng.normal(0, 2, base.shape), 0, 255).astype(np.uint8) for _ in range(Z)])
    vol[Z // 2] = 0                                                   # the blank slice
    kw = dict(gap_closing=1, min_z_extent=2)
    gen = dict(pred_iou_thresh=0.5, stability_score_thresh=0.5)          # a few hundred objects per slice on this tile
    sync = torch.cuda.synchronize

    def device_route(v):
        amg = AutomaticMaskGenerator(predictor)
        sync()
        t0 = time.perf_counter()
        labels, _ = M._segment_slices_pipelined(v, predictor, amg, 8, 3, True, gen)
        sync()
        t1 = time.perf_counter()
        merged = M.merge_instance_segmentation_3d(labels, **kw)
        out = util.fetch_to_host(merged, tag="merge3d").view(np.uint32)
        sync()
        return out, labels, t1 - t0, time.perf_counter() - t1

    def host_route(v):
        amg = AutomaticMaskGenerator(predictor)
        sync()
        t0 = time.perf_counter()
        seg, _ = M.segment_slices(v, predictor, amg, batch_size=8, **gen)
        sync()
        t1 = time.perf_counter()
        merged = M.merge_instance_segmentation_3d(seg, device=dev, **kw)
        sync()
        return merged, t1 - t0, time.perf_counter() - t1

    device_route(vol[:8])                                             # warm-up: lane streams, page-locked buffers, code objects
    host_route(vol[:4])
    rep["device_route"] = []
    for _ in range(3):
        out_d, labels, ts, tm = device_route(vol)
        rep["device_route"].append({"segment_s": round(ts, 4), "merge_s": round(tm, 4)})
        print("device route", rep["device_route"][-1], flush=True)
    rep["objects_in_slices_0_mid_last"] = [int((torch.unique(labels[z]) != 0).sum()) for z in (0, Z // 2, Z - 1)]
    lim = int(labels.max()) + 1
    ops.close_gaps_z(labels, 1, id_limit=lim)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    rep["close_gaps_ms_incl_workspace_alloc"] = []
    for _ in range(5):
        e0.record()
        closed, result = ops.close_gaps_z(labels, 1, id_limit=lim)
        e1.record()
        sync()
        rep["close_gaps_ms_incl_workspace_alloc"].append(round(e0.elapsed_time(e1), 3))
    rep["close_gaps_result"] = result.tolist()
    st = {}
    t = time.perf_counter()
    zr, _ = ops.label_z_ranges(closed, int(closed.max()) + 1)
    bool(((zr[:, 1] >= 0) & (zr[:, 0] != zr[:, 1])).any())
    st["z_ranges_and_check_s"] = round(time.perf_counter() - t, 4)
    t = time.perf_counter()
    table = ops.slice_overlaps(closed)
    st["slice_overlaps_s"] = round(time.perf_counter() - t, 4)
    uv, ov = M.edges_from_overlap_table(table)
    t = time.perf_counter()
    M._solve_node_labels(int(closed.max()) + 1, uv, ov, True)
    st["host_multicut_s"] = round(time.perf_counter() - t, 4)
    st["edges"], st["nodes"] = int(len(uv)), int(closed.max()) + 1
    rep["device_merge_stages"] = st
    rep["host_route"] = []
    for _ in range(args.host_reps):
        out_h, ts, tm = host_route(vol)
        rep["host_route"].append({"segment_s": round(ts, 4), "merge_s": round(tm, 4)})
        print("host route", rep["host_route"][-1], flush=True)
    t = time.perf_counter()
    closed_h = M._preprocess_closing(labels.cpu().numpy().view(np.uint32), 1)
    rep["host_preprocess_closing_s"] = round(time.perf_counter() - t, 3)
    rep["closing_equal"] = bool(np.array_equal(closed_h, closed.cpu().numpy()))
    rep["routes_equal"] = bool(np.array_equal(out_d, out_h))
    rep["objects_after_merge"] = int(len(np.unique(out_h)) - 1)
    line = json.dumps(rep)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
