"""generate()'s tail after the two-level component labelling (csrc/segment.hip: tile labelling in LDS, border unions, one compression
with an edge check) and the valid-limited selection (csrc/amgselect.hip: sorts and NMS over the V leading candidates only): root keys,
numbering and label images identical to the CPU oracle (oracle/amg_ref.py), never to another device path alone."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (37, 45), (64, 64), (513, 520), (1024, 1024)]       # one tile and less; ragged tiles across the 512-block border; bench size
PATTERNS = ["background", "one_value", "checkerboard", "stripes", "spiral", "comb", "diagonal", "blobs"]


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def spiral(h, w):
    """A one-pixel-wide rectangular spiral of value 1 from the outer border to the centre: ring k (inset 2k) is cut below its upper left
    corner and tied to the next ring there, so the whole image is ONE component whose first pixel is (0, 0)."""
    s = np.zeros((h, w), dtype=np.int64)
    k = 0
    while k <= h - 1 - k and k <= w - 1 - k:
        y1, x1 = h - 1 - k, w - 1 - k
        s[k, k:x1 + 1] = 1; s[y1, k:x1 + 1] = 1; s[k:y1 + 1, k] = 1; s[k:y1 + 1, x1] = 1
        if k > 0:
            s[k, k - 1] = 1                  # the tie from the previous ring's left side
            s[k - 1, k - 2] = 0              # ... whose way up to its own corner is cut
        k += 2
    return s


def pattern(name, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    if name == "background":
        return np.zeros((h, w), dtype=np.int64)
    if name == "one_value":
        return np.full((h, w), 3, dtype=np.int64)
    if name == "checkerboard":                # no 4-edge at all
        return ((yy + xx) % 2 == 0) * 2
    if name == "stripes":                     # vertical, two alternating values
        return 1 + (xx // max(1, w // 40)) % 2
    if name == "spiral":
        return spiral(h, w)
    if name == "comb":                        # teeth in every other column, joined in the last row only
        s = np.zeros((h, w), dtype=np.int64)
        s[:, ::2] = 4
        s[-1, :] = 4
        return s
    if name == "diagonal":                    # two regions of one value that touch at a corner only
        s = np.zeros((h, w), dtype=np.int64)
        s[:h // 2, :w // 2] = 5
        s[h // 2:, w // 2:] = 5
        return s
    rng = np.random.default_rng(h * 1000 + w)
    s = np.zeros((h, w), dtype=np.int64)
    for _ in range(60):
        cy, cx, r = rng.integers(0, h), rng.integers(0, w), rng.integers(1, max(2, min(h, w) // 6))
        s[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = rng.integers(1, 6)
    return s


@functools.lru_cache(maxsize=None)
def case(name, shape):
    """(label image, the oracle's numbering of it, block-major keys): computed once, shared and never modified."""
    from oracle import amg_ref as A
    seg = np.ascontiguousarray(pattern(name, *shape)).astype(np.int64)
    ref = A.label_components(seg.astype("uint32")).astype(np.int64)
    keys = A.block_major_keys(*shape).reshape(-1)
    for a in (seg, ref, keys):
        a.setflags(write=False)
    return seg, ref, keys


def check_roots(roots, seg, ref, keys):
    """roots == the oracle's labelling: -1 on the background, the same partition in the same numbering order, and every root key is the
    smallest block-major key of its component."""
    fg = seg.reshape(-1) != 0
    assert roots.shape == fg.shape and (roots[~fg] == -1).all()
    if not fg.any():
        return
    uniq, inv = np.unique(roots[fg], return_inverse=True)
    assert np.array_equal(inv + 1, ref.reshape(-1)[fg])
    first = np.full(len(uniq), np.iinfo(np.int64).max)
    np.minimum.at(first, inv, keys[fg])
    assert np.array_equal(uniq, first)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_two_level_labelling_is_the_oracles(shape):
    _gpu()
    from micro_sam_amd import ops
    for name in PATTERNS:
        seg, ref, keys = case(name, shape)
        t = torch.tensor(seg, dtype=torch.int32).cuda()
        roots = ops.label_components(t).cpu().numpy().astype(np.int64)
        check_roots(roots, seg, ref, keys)
        for passes in ((2, 1, 3) if name in ("spiral", "comb") else (2,)):
            r, flag = ops.label_components_async(t, passes=passes)
            assert int(flag.item()) == 0, (name, passes)
            assert np.array_equal(r.cpu().numpy(), roots), (name, passes)      # the argument is kept for the ABI only


# ---- selection / NMS: rectangles as masks on a 96 x 96 image
H = W = 96


def _rects(n, rng):
    """n rectangles [n, H, W] bool; sizes and places vary so that some overlap strongly (NMS) and some not at all."""
    m = np.zeros((n, H, W), dtype=bool)
    for i in range(n):
        hh, ww = rng.integers(3, 30), rng.integers(3, 30)
        y0, x0 = rng.integers(0, H - hh + 1), rng.integers(0, W - ww + 1)
        m[i, y0:y0 + hh, x0:x0 + ww] = True
    return m


def _oracle_generate(masks, iou, stab, boxes, kw):
    """The CPU restatement: threshold / crop-edge filters, greedy NMS over the valid ones in stable descending score order
    (oracle.amg_ref.nms), mask_data_to_segmentation of the survivors."""
    from oracle import amg_ref as A
    valid = np.ones(len(iou), dtype=bool)
    if kw["pred_iou_thresh"] > 0:
        valid &= iou > np.float32(kw["pred_iou_thresh"])
    if kw["stability_score_thresh"] > 0:
        valid &= stab >= np.float32(kw["stability_score_thresh"])
    valid &= ~A.is_box_near_crop_edge(torch.as_tensor(boxes), [0, 0, W, H], [0, 0, W, H]).numpy()
    idx = np.nonzero(valid)[0]
    keep = idx[A.nms(torch.as_tensor(boxes[idx]).float(), torch.as_tensor(iou[idx]), kw["box_nms_thresh"]).numpy()] if len(idx) else idx
    keep = np.sort(keep)                     # mask_data_to_segmentation sorts by area, stable: candidate order breaks ties
    recs = [{"segmentation": masks[i], "area": int(masks[i].sum())} for i in keep]
    return A.mask_data_to_segmentation(recs, shape=(H, W), with_background=kw["with_background"], merge_exclusively=False,
                                       min_object_size=kw.get("min_object_size", 0))


def _selection_case(name):
    """(masks, iou, stability, kwargs) of one named case; N and the number V of valid candidates are what the case is about."""
    rng = np.random.default_rng(sum(map(ord, name)))
    kw = dict(pred_iou_thresh=0.5, stability_score_thresh=0.5, box_nms_thresh=0.7, with_background=True)
    n = {"n1": 1, "n63": 63, "n64": 64, "n65": 65}.get(name, 130)
    masks = _rects(n, rng)
    iou = (rng.integers(55, 100, size=n) / 100).astype(np.float32)                 # all above the threshold, many ties
    stab = np.full(n, 0.9, dtype=np.float32)
    if name == "none_valid":
        iou[:] = 0.3
    elif name == "all_valid":
        kw.update(pred_iou_thresh=0.0, stability_score_thresh=0.0)
    elif name == "v64_of_130":
        stab[rng.permutation(n)[64:]] = 0.1                                        # exactly 64 pass
    elif name == "score_ties":
        iou[:] = np.float32(0.8)                                                   # every score equal: valid next to invalid, valid next to valid
        stab[::3] = 0.1
        iou[5], iou[6], iou[7] = 0.9, 0.9, 0.3                                     # (and an invalid one whose raw score ties with nothing)
    elif name == "area_ties":
        yy = (np.arange(n) // 12) * 9
        xx = (np.arange(n) % 12) * 8
        masks[:] = False
        for i in range(n):                                                        # equal-sized rectangles on a grid, neighbours overlap by a strip
            masks[i, yy[i]:yy[i] + 8, xx[i]:xx[i] + 9 + (i % 2)] = True
        kw.update(box_nms_thresh=0.9)
    return masks, iou, stab, kw


@pytest.mark.parametrize("name", ["n1", "n63", "n64", "n65", "n130", "none_valid", "all_valid", "v64_of_130", "score_ties", "area_ties"])
def test_valid_limited_selection_is_the_operator_formulation_and_the_oracle(name):
    _gpu()
    from micro_sam_amd import ops
    from micro_sam_amd._vendored import batched_mask_to_box, pack_bits
    from micro_sam_amd.instance_segmentation import AutomaticMaskGenerator, DeviceMaskData
    masks, iou, stab, kw = _selection_case(name)
    n = len(iou)
    m = torch.as_tensor(masks).cuda()
    boxes = batched_mask_to_box(m).to(torch.int32)
    area = m.flatten(1).sum(1).to(torch.int32)
    data = DeviceMaskData(mask_size=(H, W), full_size=(H, W), iou_preds=torch.as_tensor(iou).cuda(), points=torch.zeros(n, 2))
    data["stability_score"] = torch.as_tensor(stab).cuda()
    data["boxes"], data["area"], data["bits"] = boxes, area, pack_bits(m)
    amg = AutomaticMaskGenerator.__new__(AutomaticMaskGenerator)
    amg._is_initialized, amg._crop_list, amg._crop_boxes, amg._original_size = True, [data], [[0, 0, W, H]], (H, W)
    lab_f, flag_f = ops.amg_generate_labels(data["iou_preds"], data["stability_score"], boxes, area, data["bits"], (H, W), [0, 0, W, H],
                                            kw["pred_iou_thresh"], kw["stability_score_thresh"], kw["box_nms_thresh"],
                                            with_background=kw["with_background"])
    amg._torch_glue_generate = True
    lab_t, flag_t = amg.generate_device(**kw)
    assert int(flag_f.item()) == 0 and int(flag_t.item()) == 0
    assert lab_f.dtype == torch.int32 and torch.equal(lab_f, lab_t)
    ref = _oracle_generate(masks, iou, stab, boxes.cpu().numpy(), kw)
    got = lab_f.cpu().numpy()
    assert np.array_equal(got.astype(np.int64), np.asarray(ref).astype(np.int64)), f"{(got != ref).sum()} pixels differ"
    if name == "none_valid":
        assert got.max() == 0
    else:
        assert got.max() >= 1 or n == 1
