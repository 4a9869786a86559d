"""Automatic mask generation behind the reference's API: ``AMGBase`` / ``AutomaticMaskGenerator``
(``micro_sam/instance_segmentation.py:65-530``) with the expensive ``initialize`` running on libmsam_hip.so.

Differences to the reference are internal only:
* the grid prompts of a crop are decoded in device chunks (``device_chunk`` prompts, default all 1024 at once; prompts
  are independent, so the result per prompt does not depend on the chunking - ``points_per_batch`` only sets the
  progress-bar granularity); each chunk goes low-res logits -> (stability counts, boxes, areas, bit masks) on the
  device; the [64,3,H,W] fp32 logits and bool masks the reference materialises never exist;
* the initialised state stays in HBM (``DeviceMaskData``: bit masks [N, H/32, W] instead of RLE lists); the reference's
  ``"rles"`` column is produced lazily by the HIP RLE kernels the first time it is read (state pickling, ``rle`` /
  ``binary_mask`` output); ``generate(output_mode="instance_segmentation")`` paints + labels on the device;
* crops (``crop_n_layers > 0``) and tiles (``TiledAutomaticMaskGenerator``) decode at crop resolution and KEEP their bit
  masks at crop resolution in the state (``DeviceMaskData.crop_box``): 3072 candidates x 128 KiB per 1024^2 tile, however
  large the image is.  ``msam_uncrop_bits`` (the reference's ``uncrop_masks``) places only the candidates that survive
  ``_postprocess_batch`` into full-image bit masks (``generate``), and the lazily produced ``"rles"`` column uncrops in
  chunks of 256 masks (the reference pads every candidate to the full image before it filters: O(192 H W) per batch,
  micro_sam/instance_segmentation.py:250).
"""
from __future__ import annotations

from abc import ABC
from copy import deepcopy
from typing import Any, Dict, List, Optional, Union

import numpy as np
import torch

from . import _lib, amg_utils, ops, util
from ._prompt_prefix import PromptPrefixCache
from .predictor import SamPredictor


class DeviceMaskData(amg_utils.MaskData):
    """``MaskData`` whose masks live on the device as bit masks (column ``"bits"`` + ``"mask_size"``).

    ``data["rles"]`` (the reference's column) is materialised on first access by the HIP RLE kernels and cached;
    ``filter`` / ``cat`` keep both representations consistent."""

    def __init__(self, mask_size=None, crop_box=None, full_size=None, **kwargs) -> None:
        super().__init__(**kwargs)
        self.mask_size = mask_size          # resolution of the "bits" column
        self.crop_box = crop_box            # [x0, y0, x1, y1] when the bits are at crop resolution, else None
        self.full_size = full_size          # (H, W) of the image the crop belongs to

    def _is_cropped(self) -> bool:
        return self.crop_box is not None and self.full_size is not None and tuple(self.mask_size) != tuple(self.full_size)

    def full_bits(self, bits: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The (given rows of the) bit masks at full-image resolution (``uncrop_masks``)."""
        bits = self._stats["bits"] if bits is None else bits
        if not self._is_cropped():
            return bits
        return ops.uncrop_bits(bits.contiguous(), self.crop_box, self.full_size[0], self.full_size[1])

    def __getitem__(self, key: str):
        if key == "rles" and "rles" not in self._stats and "bits" in self._stats:
            self._stats["rles"] = self._encode_rles()
        return self._stats[key]

    def _encode_rles(self):
        bits = self._stats["bits"]
        if bits.shape[0] == 0:
            return []
        if not self._is_cropped():
            h, w = self.mask_size
            counts, offsets = ops.rle_encode(bits.contiguous(), h, w)
            return ops.rles_to_list(counts, offsets, h, w, as_list=False)
        # RLEs are those of the masks padded to the full image (the reference's uncrop_masks precedes its RLE encoding):
        # uncrop a bounded chunk at a time
        h, w = self.full_size
        out = []
        for s in range(0, bits.shape[0], 256):
            counts, offsets = ops.rle_encode(self.full_bits(bits[s:s + 256]), h, w)
            out.extend(ops.rles_to_list(counts, offsets, h, w, as_list=False))
        return out

    def shallow_copy(self) -> "DeviceMaskData":
        out = DeviceMaskData(mask_size=self.mask_size, crop_box=self.crop_box, full_size=self.full_size)
        out._stats = dict(self._stats)
        return out

    def cat(self, new_stats) -> None:
        new_cropped = isinstance(new_stats, DeviceMaskData) and new_stats._is_cropped()
        same_crop = new_cropped and self.crop_box is not None and list(self.crop_box) == list(new_stats.crop_box)
        if "rles" in self._stats and "rles" not in new_stats._stats and "bits" in new_stats._stats:
            new_stats["rles"]                      # materialise so that both sides carry the column
        if new_cropped and not same_crop:
            # joining the (filtered) masks of a crop / tile to full-image data: place them in full-image bit masks now
            items = dict(new_stats.items())
            if "bits" in items:
                items["bits"] = new_stats.full_bits()
            self.mask_size, self.crop_box = tuple(new_stats.full_size), None
            self.full_size = tuple(new_stats.full_size)
        else:
            items = dict(new_stats.items())
            if getattr(new_stats, "mask_size", None) is not None:
                self.mask_size = new_stats.mask_size
                if same_crop or (isinstance(new_stats, DeviceMaskData) and "bits" not in self._stats):
                    self.crop_box, self.full_size = new_stats.crop_box, new_stats.full_size
        for k, v in items.items():
            cur = self._stats.get(k)
            if cur is None:
                self._stats[k] = v                 # columns are never mutated in place: no deep copy needed
            elif isinstance(v, torch.Tensor):
                self._stats[k] = torch.cat([cur, v.to(cur.device)], dim=0)
            elif isinstance(v, np.ndarray):
                self._stats[k] = np.concatenate([cur, v], axis=0)
            else:
                self._stats[k] = cur + list(v)

    def __len__(self) -> int:
        return int(self._stats["iou_preds"].shape[0]) if "iou_preds" in self._stats else 0

    def __getstate__(self):
        """Pickle in the reference's format: RLE dicts on the host instead of device bit masks."""
        stats = {}
        for k, v in self._stats.items():
            if k == "bits":
                continue
            stats[k] = v.cpu() if torch.is_tensor(v) else v
        if "bits" in self._stats:
            stats["rles"] = self["rles"]
        size = self.full_size if self._is_cropped() else self.mask_size
        return {"_stats": stats, "mask_size": size}

    def __setstate__(self, state):
        self._stats = state["_stats"]
        self.mask_size = state["mask_size"]
        self.crop_box = None
        self.full_size = state["mask_size"]


DEFAULT_SEGMENTATION_MODE_WITH_DECODER = "ais"       # reference :44


class AMGBase(ABC):
    def __init__(self):
        self._is_initialized = False
        self._crop_list = None
        self._crop_boxes = None
        self._original_size = None

    @property
    def is_initialized(self):
        return self._is_initialized

    @property
    def crop_list(self):
        return self._crop_list

    @property
    def crop_boxes(self):
        return self._crop_boxes

    @property
    def original_size(self):
        return self._original_size

    def _postprocess_batch(self, data, crop_box, original_size, pred_iou_thresh, stability_score_thresh, box_nms_thresh):
        orig_h, orig_w = original_size
        # The reference filters the columns three times (predicted IoU, stability, crop edge) and once more by the NMS result
        # (:106-133).  The three tests are independent of each other, so they are ANDed here and every column is gathered ONCE with
        # the final index list (survivors of the tests, in NMS order): same rows in the same order, one host synchronisation per crop
        # instead of one per column and test (boolean indexing of a device tensor waits for its count).
        keep = ~amg_utils.is_box_near_crop_edge(data["boxes"], crop_box, [0, 0, orig_w, orig_h])
        if pred_iou_thresh > 0.0:
            keep = keep & (data["iou_preds"] > pred_iou_thresh).to(keep.device)
        if stability_score_thresh > 0.0:
            keep = keep & (data["stability_score"] >= stability_score_thresh).to(keep.device)
        idx = torch.nonzero(keep).squeeze(1)
        boxes, scores = data["boxes"][idx], data["iou_preds"][idx]
        if boxes.is_cuda:
            keep_by_nms = ops.box_nms(boxes, scores, box_nms_thresh)                         # one category
        else:
            keep_by_nms = amg_utils.batched_nms(boxes.float(), scores, torch.zeros_like(boxes[:, 0]), iou_threshold=box_nms_thresh)
        data.filter(idx[keep_by_nms.to(idx.device)])
        data["boxes"] = amg_utils.uncrop_boxes_xyxy(data["boxes"], crop_box)
        data["crop_boxes"] = torch.tensor([crop_box for _ in range(int(data["iou_preds"].shape[0]))])
        try:
            data["points"] = amg_utils.uncrop_points(data["points"], crop_box)
        except KeyError:
            pass
        return data

    def _postprocess_batch_prepare(self, data, crop_box, original_size, pred_iou_thresh, stability_score_thresh, box_nms_thresh):
        """The tests of ``_postprocess_batch`` for a device state WITHOUT a host synchronisation: returns (order, count) - the rows that
        survive the three filters and the box NMS are ``order[:count]``, in the order ``_postprocess_batch`` leaves them (descending
        predicted IoU, ties by row).  ``generate`` prepares every crop / tile first and reads all counts in one transfer (round 5: a
        2048^2 slice has 9 tiles, two synchronisations each were 6 of its generate()'s 9 ms)."""
        orig_h, orig_w = original_size
        keep = ~amg_utils.is_box_near_crop_edge(data["boxes"], crop_box, [0, 0, orig_w, orig_h])
        if pred_iou_thresh > 0.0:
            keep = keep & (data["iou_preds"] > pred_iou_thresh)
        if stability_score_thresh > 0.0:
            keep = keep & (data["stability_score"] >= stability_score_thresh)
        scores = data["iou_preds"].float()
        flags = ops.box_nms_flags(data["boxes"], scores, keep, box_nms_thresh)
        order = torch.sort(torch.where(flags, scores, torch.full_like(scores, float("-inf"))), descending=True, stable=True).indices
        return order, flags.sum()

    def _postprocess_batch_finish(self, data, crop_box, order, count: int):
        data.filter(order[:count])
        data["boxes"] = amg_utils.uncrop_boxes_xyxy(data["boxes"], crop_box)
        data["crop_boxes"] = torch.tensor([crop_box for _ in range(int(data["iou_preds"].shape[0]))])
        try:
            data["points"] = amg_utils.uncrop_points(data["points"], crop_box)
        except KeyError:
            pass
        return data

    def _postprocess_small_regions(self, mask_data, min_area, nms_thresh):
        """Reference :146-186: remove small islands / fill small holes of every kept mask (host step, like the reference's
        cv2 loop), recompute boxes, NMS that prefers unchanged masks, re-encode the changed ones."""
        from ._vendored import batched_mask_to_box
        rles = list(mask_data["rles"])
        if len(rles) == 0:
            return mask_data
        for k in ("bits", "area"):                 # device columns go stale below: continue with the reference's columns
            if k in mask_data:
                del mask_data[k]
        mask_data["rles"] = rles
        new_masks, scores = [], []
        for rle in rles:
            mask = amg_utils.rle_to_mask(rle)
            mask, changed = amg_utils.remove_small_regions(mask, min_area, mode="holes")
            unchanged = not changed
            mask, changed = amg_utils.remove_small_regions(mask, min_area, mode="islands")
            unchanged = unchanged and not changed
            new_masks.append(torch.as_tensor(mask, dtype=torch.int).unsqueeze(0))
            scores.append(float(unchanged))
        masks = torch.cat(new_masks, dim=0)
        boxes = batched_mask_to_box(masks.to(torch.bool))
        keep_by_nms = amg_utils.batched_nms(boxes.float(), torch.as_tensor(scores, dtype=torch.float),
                                            torch.zeros_like(boxes[:, 0]), iou_threshold=nms_thresh)
        box_col = torch.as_tensor(mask_data["boxes"]).clone()
        for i_mask in keep_by_nms.tolist():
            if scores[i_mask] == 0.0:
                mask_data["rles"][i_mask] = amg_utils.mask_to_rle_numpy(masks[i_mask].numpy().astype(bool))
                box_col[i_mask] = boxes[i_mask].to(box_col.dtype)
        mask_data["boxes"] = box_col.numpy() if isinstance(mask_data["boxes"], np.ndarray) else box_col
        mask_data.filter(keep_by_nms)
        return mask_data

    def _postprocess_masks(self, mask_data, min_mask_region_area, box_nms_thresh, crop_nms_thresh, output_mode):
        if min_mask_region_area > 0:
            mask_data = self._postprocess_small_regions(mask_data, min_mask_region_area, max(box_nms_thresh, crop_nms_thresh))
        if output_mode == "coco_rle":
            mask_data["segmentations"] = [amg_utils.coco_encode_rle(rle) for rle in mask_data["rles"]]
        elif output_mode in ("binary_mask", "instance_segmentation"):
            if "bits" in mask_data:
                h, w = mask_data.mask_size
                dense = ops.unpack_bits(torch.as_tensor(mask_data["bits"]), h).cpu().numpy()
                mask_data["segmentations"] = [m for m in dense]
            else:
                mask_data["segmentations"] = [amg_utils.rle_to_mask(rle) for rle in mask_data["rles"]]
        elif output_mode == "rle":
            mask_data["segmentations"] = [{"size": r["size"], "counts": np.asarray(r["counts"]).tolist()}
                                          for r in mask_data["rles"]]
        else:
            raise ValueError(f"Invalid output mode {output_mode}.")
        curr_anns = []
        for idx in range(len(mask_data["segmentations"])):
            ann = {
                "segmentation": mask_data["segmentations"][idx],
                "area": int(mask_data["area"][idx]) if "area" in mask_data else amg_utils.area_from_rle(mask_data["rles"][idx]),
                "bbox": amg_utils.box_xyxy_to_xywh(mask_data["boxes"][idx]).tolist(),
                "predicted_iou": mask_data["iou_preds"][idx].item(),
                "stability_score": mask_data["stability_score"][idx].item(),
                "crop_box": amg_utils.box_xyxy_to_xywh(mask_data["crop_boxes"][idx]).tolist(),
            }
            try:
                ann["point_coords"] = [mask_data["points"][idx].tolist()]
            except KeyError:
                pass
            curr_anns.append(ann)
        return curr_anns

    def _to_mask_data_device(self, iou_preds, post, crop_box, original_size, points=None):
        """``AMGBase._to_mask_data`` (reference :229-255) from the fused device post-processing results."""
        orig_h, orig_w = original_size
        x0, y0, x1, y1 = crop_box
        full_image = (x0 == 0 and y0 == 0 and x1 == orig_w and y1 == orig_h)
        n_masks_per_prompt = iou_preds.shape[1]
        data = DeviceMaskData(mask_size=(orig_h, orig_w) if full_image else (y1 - y0, x1 - x0),
                              crop_box=None if full_image else list(crop_box), full_size=(orig_h, orig_w),
                              iou_preds=iou_preds.flatten(0, 1))
        if points is not None:
            data["points"] = torch.as_tensor(points.repeat(n_masks_per_prompt, axis=0), dtype=torch.float)
        counts = post["counts"]
        # calculate_stability_score: #(logit > thr + off) / #(logit > thr - off); int32 / int32 -> float32 (0/0 -> nan)
        data["stability_score"] = counts[:, 0] / counts[:, 1]
        data["boxes"] = post["boxes"]
        data["area"] = counts[:, 2]                 # == area_from_rle of the mask
        # uncrop_masks: identity for the full-image crop; other crops keep their bit masks at crop resolution, only the
        # survivors of _postprocess_batch are placed in full-image bit masks (DeviceMaskData.cat / full_bits)
        data["bits"] = post["bits"]
        return data

    def get_state(self) -> Dict[str, Any]:
        if not self.is_initialized:
            raise RuntimeError("The state has not been computed yet. Call initialize first.")
        return {"crop_list": self.crop_list, "crop_boxes": self.crop_boxes, "original_size": self.original_size}

    def set_state(self, state: Dict[str, Any]) -> None:
        self._crop_list = state["crop_list"]
        self._crop_boxes = state["crop_boxes"]
        self._original_size = state["original_size"]
        self._is_initialized = True

    def clear_state(self):
        self._crop_list = None
        self._crop_boxes = None
        self._original_size = None
        self._is_initialized = False


class AutomaticMaskGenerator(AMGBase):
    """Grid-prompt instance segmentation; same constructor / ``initialize`` / ``generate`` as the reference (:288-530)."""

    def __init__(self, predictor: SamPredictor, points_per_side: Optional[int] = 32, points_per_batch: Optional[int] = None,
                 crop_n_layers: int = 0, crop_overlap_ratio: float = 512 / 1500, crop_n_points_downscale_factor: int = 1,
                 point_grids: Optional[List[np.ndarray]] = None, stability_score_offset: float = 1.0,
                 device_chunk: int = 1024):
        super().__init__()
        self._device_chunk = int(device_chunk)
        if points_per_side is not None:
            self.point_grids = amg_utils.build_all_layer_point_grids(points_per_side, crop_n_layers,
                                                                     crop_n_points_downscale_factor)
        elif point_grids is not None:
            self.point_grids = point_grids
        else:
            raise ValueError("Can't have both points_per_side and point_grid be None or not None.")
        self._predictor = predictor
        self._points_per_side = points_per_side
        self._points_per_batch = 64 if points_per_batch is None else points_per_batch
        self._crop_n_layers = crop_n_layers
        self._crop_overlap_ratio = crop_overlap_ratio
        self._crop_n_points_downscale_factor = crop_n_points_downscale_factor
        self._stability_score_offset = stability_score_offset

    def _lane_clone(self, lane_predictor: Optional[SamPredictor] = None) -> "AutomaticMaskGenerator":
        """Another generator with the same settings on a lane view of the predictor's model (own decoder scratch, own state): what a
        concurrent decode lane of the pipelined slice / tile loops works with."""
        import copy
        clone = copy.copy(self)
        clone._predictor = lane_predictor if lane_predictor is not None else SamPredictor(self._predictor.model.lane_view())
        clone._prompt_cache = PromptPrefixCache()
        clone._lanes = clone._post_stream = None
        clone.clear_state()
        return clone

    def _decode_lanes(self, n: int):
        """``n`` (lane clone, HIP stream) pairs.  The expensive part of a lane - the model view with its decoder workspace (several GiB for
        1024 prompts) and its stream (torch caches device memory per stream) - is kept on the PREDICTOR, so generators that come and go
        (one per call of a caller's loop) find it again; the clones themselves are kept on the generator.  Fresh views / streams per call
        allocated the workspaces anew every time (measured: 21 tiles/s instead of > 150)."""
        dev = self._predictor.device
        pool = getattr(self._predictor, "_lane_pool", None) or []
        if pool and (pool[0][0].device != dev or pool[0][0].model.mask_decoder is not self._predictor.model.mask_decoder):
            pool = []                              # the predictor was moved / its model replaced
        while len(pool) < n:
            pool.append((SamPredictor(self._predictor.model.lane_view()), torch.cuda.Stream(device=dev)))
        self._predictor._lane_pool = pool
        # a lane view is a shallow snapshot of the Sam object: settings changed on the main model since (set_precision,
        # set_split_token_mlp, use_glds, amg_low_res_dtype) are carried over here, and a view whose prepared decoder constants were
        # built under other settings rebuilds them (lanes could decode with other settings than the serial path)
        main = self._predictor.model
        for lp, _ in pool[:n]:
            lm, stale = lp.model, False
            for k in ("precision", "split_token_mlp", "use_glds", "amg_low_res_dtype"):
                if getattr(lm, k, None) != getattr(main, k, None):
                    setattr(lm, k, getattr(main, k))
                    stale = stale or k in ("split_token_mlp", "use_glds")
            if stale:
                lm._dec = None
                lm._img_state = None
        lanes = getattr(self, "_lanes", None) or []
        if lanes and any(l[0]._predictor is not p for l, (p, _) in zip(lanes, pool)):
            lanes = []
        while len(lanes) < n:
            lp, st = pool[len(lanes)]
            lanes.append((self._lane_clone(lp), st))
        self._lanes = lanes
        for clone, _ in lanes[:n]:                 # settings may have been changed on the generator since the clone was made
            for k in ("point_grids", "_points_per_side", "_points_per_batch", "_crop_n_layers", "_crop_overlap_ratio",
                      "_crop_n_points_downscale_factor", "_stability_score_offset", "_device_chunk"):
                setattr(clone, k, getattr(self, k))
        return lanes[:n]

    def _process_batch(self, points, im_size, crop_box, original_size):
        # the grid prompts of a crop size are the same for every image: keep their device copy (one H2D copy and one fill
        # less per tile - each is a separate, serialising command on the stream) and, on the kernel path, the part of the
        # decode that reads nothing else (Sam.make_prompt_prefix: 7 launches less per tile).  The knob is read HERE, once per
        # call (msam_tune_set("prompt_prefix", 0): no block is kept and every decode runs those launches itself)
        predictor = self._predictor
        model = predictor.model
        with_prefix = not model.reference_formulation and _lib.tune_get("prompt_prefix") == 1
        # the blocks belong to the decoder's prepared constants: another object (new weights, settings, a PEFT merge) drops them all
        owner = model._prepare_decoder() if with_prefix else None
        device = predictor.device

        def make(pts_host):
            transformed_points = predictor.transform.apply_coords(pts_host, im_size)
            in_points = torch.as_tensor(transformed_points, device=device, dtype=torch.float)
            in_labels = torch.ones(in_points.shape[0], dtype=torch.int, device=in_points.device)
            prefix = model.make_prompt_prefix(in_points[:, None, :], in_labels[:, None]) if with_prefix else None
            return in_points, in_labels, prefix

        if getattr(self, "_prompt_cache", None) is None:
            self._prompt_cache = PromptPrefixCache()
        key = (points.shape, tuple(im_size), float(points[0, 0]), float(points[-1, -1]), str(device), with_prefix)
        in_points, in_labels, prefix = self._prompt_cache.get(key, points, owner, make)
        if prefix is not None:
            iou_preds, post = predictor.predict_masks_device(None, None, multimask_output=True,
                                                             stability_score_offset=self._stability_score_offset,
                                                             prompt_prefix=prefix)
        else:
            iou_preds, post = predictor.predict_masks_device(
                in_points[:, None, :], in_labels[:, None], multimask_output=True,
                stability_score_offset=self._stability_score_offset)
        return self._to_mask_data_device(iou_preds, post, crop_box, original_size, points=points)

    def _process_crop(self, image, crop_box, crop_layer_idx, precomputed_embeddings, pbar_init=None, pbar_update=None):
        x0, y0, x1, y1 = crop_box
        cropped_im = image[y0:y1, x0:x1, :]
        cropped_im_size = cropped_im.shape[:2]
        if not precomputed_embeddings:
            self._predictor.set_image(cropped_im)
        points_scale = np.array(cropped_im_size)[None, ::-1]
        points_for_image = self.point_grids[crop_layer_idx] * points_scale
        full_image = (x0 == 0 and y0 == 0 and (y1, x1) == tuple(self.original_size))
        data = DeviceMaskData(mask_size=tuple(self.original_size) if full_image else tuple(cropped_im_size),
                              crop_box=None if full_image else list(crop_box), full_size=tuple(self.original_size))
        n_batches = len(points_for_image) // self._points_per_batch + \
            int(len(points_for_image) % self._points_per_batch != 0)
        if pbar_init is not None:
            pbar_init(n_batches, "Predict masks for point grid prompts")
        # prompts are independent: decode them in large device chunks (same per-prompt results as 64 at a time)
        chunk = max(self._device_chunk, self._points_per_batch)
        for (points,) in amg_utils.batch_iterator(chunk, points_for_image):
            batch_data = self._process_batch(points, cropped_im_size, crop_box, self.original_size)
            data.cat(batch_data)
            del batch_data
            if pbar_update is not None:
                pbar_update(int(np.ceil(len(points) / self._points_per_batch)))
        if not precomputed_embeddings:
            self._predictor.reset_image()
        return data

    @torch.no_grad()
    def initialize(self, image: np.ndarray, image_embeddings=None, i: Optional[int] = None, verbose: bool = False,
                   pbar_init: Optional[callable] = None, pbar_update: Optional[callable] = None) -> None:
        original_size = image.shape[:2]
        self._original_size = original_size
        crop_boxes, layer_idxs = amg_utils.generate_crop_boxes(original_size, self._crop_n_layers,
                                                               self._crop_overlap_ratio)
        if len(crop_boxes) == 1:
            if image_embeddings is None:
                image_embeddings = util.precompute_image_embeddings(self._predictor, image, verbose=verbose)
            util.set_precomputed(self._predictor, image_embeddings, i=i)
            precomputed_embeddings = True
        else:
            precomputed_embeddings = False
        if precomputed_embeddings:
            # with precomputed embeddings only the image SHAPE is used below (the reference converts the image with
            # util._to_image regardless); skip the host-side conversion of the pixel data
            image = np.broadcast_to(np.zeros((1, 1, 1), dtype=np.uint8), tuple(original_size) + (3,))
        else:
            image = util._to_image(image)
        _, pbar_init, pbar_update, pbar_close = util.handle_pbar(verbose, pbar_init, pbar_update)
        crop_list = []
        for crop_box, layer_idx in zip(crop_boxes, layer_idxs):
            crop_list.append(self._process_crop(image, crop_box, layer_idx, precomputed_embeddings=precomputed_embeddings,
                                                pbar_init=pbar_init, pbar_update=pbar_update))
        pbar_close()
        self._is_initialized = True
        self._crop_list = crop_list
        self._crop_boxes = crop_boxes

    @torch.no_grad()
    def generate_device(self, pred_iou_thresh: float = 0.88, stability_score_thresh: float = 0.95,
                        box_nms_thresh: float = 0.7, with_background: bool = True, min_object_size: int = 0,
                        stream: Optional["torch.cuda.Stream"] = None):
        """``generate(output_mode="instance_segmentation")`` without a single host synchronisation: threshold filters as one
        boolean vector, device NMS on the valid subset, paint + connected components + relabel on the device.

        Returns (labels int32 [H,W] device tensor, flag int32[1] that reads 0 when the labelling converged).
        Identical labels to ``generate()`` (same filters in the same order, same stable sorts).

        ``stream``: run on this side stream (after everything enqueued so far on the current stream, i.e. after the
        ``initialize`` that produced the state).  ``generate`` is a chain of ~60 small, latency-bound launches (one-wave NMS
        sweep, union-find passes, scans over one label image) that leave the chip almost empty; on a side stream they run
        underneath the next tile's decoder kernels instead of in front of them.  The state tensors are marked as in use by
        that stream (``record_stream``) so that the next ``initialize`` cannot recycle their memory early; the CALLER must
        make the consumer of the results wait for ``stream`` (``torch.cuda.current_stream().wait_stream(stream)``)."""
        if not self.is_initialized:
            raise RuntimeError("AutomaticMaskGenerator has not been initialized. Call initialize first.")
        if len(self.crop_list) != 1 or "bits" not in self.crop_list[0]:
            raise RuntimeError("generate_device needs the single-crop device state produced by initialize()")
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream(stream.device))
            for k in ("iou_preds", "stability_score", "boxes", "area", "bits"):
                self.crop_list[0][k].record_stream(stream)
            with torch.cuda.stream(stream):
                return self.generate_device(pred_iou_thresh, stability_score_thresh, box_nms_thresh, with_background,
                                            min_object_size)
        data, crop_box = self.crop_list[0], self.crop_boxes[0]
        orig_h, orig_w = self.original_size
        if 0 < len(data) <= 4096 and tuple(crop_box) == (0, 0, orig_w, orig_h) and not getattr(self, "_torch_glue_generate", False):
            # the whole chain as 13 kernels of one library call (csrc/amgselect.hip); the torch-operator formulation below
            # is kept for states with more than 4096 candidates and as the cross-check of tests/test_gpu_segment.py
            return ops.amg_generate_labels(data["iou_preds"], data["stability_score"], data["boxes"], data["area"], data["bits"],
                                           self.original_size, crop_box, pred_iou_thresh, stability_score_thresh, box_nms_thresh,
                                           min_object_size=min_object_size, with_background=with_background)
        valid = torch.ones_like(data["iou_preds"], dtype=torch.bool)
        if pred_iou_thresh > 0.0:
            valid &= data["iou_preds"] > pred_iou_thresh
        if stability_score_thresh > 0.0:
            valid &= data["stability_score"] >= stability_score_thresh
        valid &= ~amg_utils.is_box_near_crop_edge(data["boxes"], crop_box, [0, 0, orig_w, orig_h])
        keep = ops.box_nms_flags(data["boxes"], data["iou_preds"], valid, box_nms_thresh)
        return util.masks_to_segmentation_device(data["bits"], data["area"], keep, self.original_size,
                                                 min_object_size=min_object_size, with_background=with_background)

    @torch.no_grad()
    def generate(self, pred_iou_thresh: float = 0.88, stability_score_thresh: float = 0.95, box_nms_thresh: float = 0.7,
                 crop_nms_thresh: float = 0.7, min_mask_region_area: int = 0, output_mode: str = "instance_segmentation",
                 with_background: bool = True) -> Union[List[Dict[str, Any]], np.ndarray]:
        if not self.is_initialized:
            raise RuntimeError("AutomaticMaskGenerator has not been initialized. Call initialize first.")
        if (output_mode == "instance_segmentation" and min_mask_region_area == 0 and len(self.crop_list) == 1
                and isinstance(self.crop_list[0], DeviceMaskData) and "bits" in self.crop_list[0]
                and 0 < len(self.crop_list[0]) <= 4096
                and tuple(self.crop_boxes[0]) == (0, 0, self.original_size[1], self.original_size[0])
                and not getattr(self, "_general_generate", False)):
            # the default call on a single-crop device state: the whole of _postprocess_batch + mask_data_to_segmentation as ONE
            # library call (generate_device: 13 kernels, no host synchronisation) and one download of label image + flag
            labels, flag = self.generate_device(pred_iou_thresh, stability_score_thresh, box_nms_thresh, with_background)
            out = util.fetch_to_host(torch.cat([labels.reshape(-1), flag]), tag="labels")
            if out[-1] == 0:
                return out[:-1].reshape(self.original_size).view(np.uint32)
            # (the labelling reported an open edge: the general path below repeats it under host control)
        data = DeviceMaskData()
        on_device = len(self.crop_list) > 1 and all(
            isinstance(d, DeviceMaskData) and len(d) > 0 and all(torch.is_tensor(d[k]) and d[k].is_cuda for k in ("boxes", "iou_preds", "stability_score"))
            for d in self.crop_list)
        if on_device:
            # every crop's filters + box NMS are enqueued first, their survivor counts come back in ONE transfer
            prepared = [self._postprocess_batch_prepare(d, cb, self.original_size, pred_iou_thresh, stability_score_thresh, box_nms_thresh)
                        for d, cb in zip(self.crop_list, self.crop_boxes)]
            counts = torch.stack([c for _, c in prepared]).tolist()
            for data_, crop_box, (order, _), n in zip(self.crop_list, self.crop_boxes, prepared, counts):
                data.cat(self._postprocess_batch_finish(data_.shallow_copy(), crop_box, order, int(n)))
        else:
            for data_, crop_box in zip(self.crop_list, self.crop_boxes):
                # filter() re-binds columns and never mutates them in place: a shallow copy protects the state
                crop_data = self._postprocess_batch(
                    data=data_.shallow_copy() if isinstance(data_, DeviceMaskData) else deepcopy(data_),
                    crop_box=crop_box, original_size=self.original_size,
                    pred_iou_thresh=pred_iou_thresh, stability_score_thresh=stability_score_thresh,
                    box_nms_thresh=box_nms_thresh)
                data.cat(crop_data)
        if len(self.crop_boxes) > 1 and len(data["crop_boxes"]) > 0:
            scores = 1 / amg_utils.box_area(data["crop_boxes"])
            scores = scores.to(data["boxes"].device)
            keep_by_nms = amg_utils.batched_nms(data["boxes"].float(), scores, torch.zeros_like(data["boxes"][:, 0]),
                                                iou_threshold=crop_nms_thresh)
            data.filter(keep_by_nms)
        if output_mode == "instance_segmentation" and min_mask_region_area == 0 and "bits" in data:
            # device path of util.mask_data_to_segmentation (paint by area + connected components + relabel)
            return util.mask_data_to_segmentation_device(data["bits"], data["area"], self.original_size,
                                                         with_background=with_background)
        bits = data["bits"] if "bits" in data else None
        if bits is not None:
            del data["bits"]
        data.to_numpy()
        if bits is not None:
            data["bits"] = bits                   # keep the masks on the device for unpacking
        masks = self._postprocess_masks(data, min_mask_region_area, box_nms_thresh, crop_nms_thresh, output_mode)
        if output_mode == "instance_segmentation":
            shape = next(iter(masks))["segmentation"].shape if len(masks) > 0 else self.original_size
            masks = util.mask_data_to_segmentation(masks, shape=shape, with_background=with_background,
                                                   merge_exclusively=False)
        return masks


def _process_tiled_embeddings(predictor, image, image_embeddings, tile_shape, halo, verbose, batch_size, mask, i):
    """Reference instance_segmentation.py:534-561."""
    if image_embeddings is None:
        if tile_shape is None or halo is None:
            raise ValueError("To compute tiled embeddings the parameters tile_shape and halo have to be passed.")
        image_embeddings = util.precompute_image_embeddings(predictor, image, tile_shape=tile_shape, halo=halo,
                                                            verbose=verbose, batch_size=batch_size, mask=mask)
    feats = image_embeddings["features"]
    tile_shape_, halo_ = tuple(feats.attrs["tile_shape"]), tuple(feats.attrs["halo"])
    if tile_shape is None:
        tile_shape = tile_shape_
    elif tuple(tile_shape) != tile_shape_:
        raise ValueError(f"Inconsistent tile_shape parameter {tile_shape} with precomputed embeedings: {tile_shape_}.")
    if halo is None:
        halo = halo_
    elif tuple(halo) != halo_:
        raise ValueError(f"Inconsistent halo parameter {halo} with precomputed embeedings: {halo_}.")
    tiles_in_mask = feats.attrs.get("tiles_in_mask", None)
    if tiles_in_mask is not None and i is not None:
        tiles_in_mask = tiles_in_mask[str(i)]
    return image_embeddings, tile_shape, halo, tiles_in_mask


class TiledAutomaticMaskGenerator(AutomaticMaskGenerator):
    """``AutomaticMaskGenerator`` on tiled embeddings (reference instance_segmentation.py:564-680): every tile (outer
    block = tile + halo) is a crop box with its own precomputed embedding.

    ``tile_lanes`` (not in the reference): the tiles of an image are decoded on this many concurrent lanes - lane views of the model on
    their own HIP streams, each with its own decoder workspace (~3 GiB for 1024 prompts per pass); 1 = the reference's serial loop
    with one workspace.  Same results either way."""

    def __init__(self, predictor: SamPredictor, points_per_side: Optional[int] = 32, points_per_batch: int = 64,
                 point_grids: Optional[List[np.ndarray]] = None, stability_score_offset: float = 1.0,
                 device_chunk: int = 1024, tile_lanes: int = 3) -> None:
        super().__init__(predictor=predictor, points_per_side=points_per_side, points_per_batch=points_per_batch,
                         point_grids=point_grids, stability_score_offset=stability_score_offset, device_chunk=device_chunk)
        self.tile_lanes = max(1, int(tile_lanes))

    @torch.no_grad()
    def initialize(self, image: np.ndarray, image_embeddings=None, i: Optional[int] = None,
                   tile_shape=None, halo=None, verbose: bool = False, pbar_init: Optional[callable] = None,
                   pbar_update: Optional[callable] = None, batch_size: int = 1, mask=None) -> None:
        from .tiling import Blocking
        original_size = image.shape[:2]
        self._original_size = original_size
        self._image_embeddings, tile_shape, halo, tiles_in_mask = _process_tiled_embeddings(
            self._predictor, image, image_embeddings, tile_shape, halo, verbose=verbose, batch_size=batch_size, mask=mask, i=i)
        image_embeddings = self._image_embeddings
        tiling = Blocking([0, 0], original_size, tile_shape)
        if tiles_in_mask is None:
            n_tiles = tiling.number_of_blocks
            tile_ids = range(n_tiles)
        else:
            n_tiles = len(tiles_in_mask)
            tile_ids = tiles_in_mask
        tiles = [tiling.get_block_with_halo(tile_id, list(halo)).outer_block for tile_id in tile_ids]
        crop_boxes = [[tile.begin[1], tile.begin[0], tile.end[1], tile.end[0]] for tile in tiles]
        _, pbar_init, pbar_update, pbar_close = util.handle_pbar(verbose, pbar_init, pbar_update)
        pbar_init(n_tiles, "Compute masks for tile")
        # only the image SHAPE is used below (the embeddings are precomputed): skip the host-side pixel conversion
        image = np.broadcast_to(np.zeros((1, 1, 1), dtype=np.uint8), tuple(original_size) + (3,))
        mask_data = []
        # round 4: the tiles of one image are decoded on `tile_lanes` concurrent lanes (lane clones on their own HIP streams, as in the
        # pipelined slice loop): the kernels of different tiles overlap instead of running one tile after the other.  Every lane waits for
        # an event recorded on the caller's stream first (whatever produced / still reads the previous state is ordered before it), the
        # caller's stream waits for all lanes at the end: the state is complete when initialize returns, as in the serial loop.
        n_lanes = min(int(getattr(self, "tile_lanes", 3)), n_tiles)
        lanes = None
        if n_lanes > 1 and str(self._predictor.device).startswith("cuda") and torch.cuda.is_available() \
                and hasattr(self._predictor.model, "lane_view"):
            lanes = self._decode_lanes(n_lanes)
            main = torch.cuda.current_stream(self._predictor.device)
            start = torch.cuda.Event()
            start.record(main)
        for idx, tile_id in enumerate(tile_ids):
            features = image_embeddings["features"][str(tile_id)]
            tile_embeddings = {"features": features, "input_size": features.attrs["input_size"],
                               "original_size": features.attrs["original_size"]}
            if lanes is None:
                util.set_precomputed(self._predictor, tile_embeddings, i)
                mask_data.append(self._process_crop(image, crop_box=crop_boxes[idx], crop_layer_idx=0,
                                                    precomputed_embeddings=True))
            else:
                clone, st = lanes[idx % n_lanes]
                clone._original_size = original_size
                st.wait_event(start)
                with torch.cuda.stream(st):
                    util.set_precomputed(clone._predictor, tile_embeddings, i)
                    mask_data.append(clone._process_crop(image, crop_box=crop_boxes[idx], crop_layer_idx=0,
                                                         precomputed_embeddings=True))
            pbar_update(1)
        if lanes is not None:
            for _, st in lanes[:n_lanes]:
                main.wait_stream(st)
            util.set_precomputed(self._predictor, tile_embeddings, i)        # the predictor holds the last tile, as after the serial loop
        pbar_close()
        self._is_initialized = True
        self._crop_list = mask_data
        self._crop_boxes = crop_boxes


# ---------------------------------------------------------------------------------------------------------------
# Segmentation from a decoder's foreground / distance maps (reference :688-1628)
# ---------------------------------------------------------------------------------------------------------------

def _get_centers(segmentation: np.ndarray, avoid_image_border: bool = True) -> np.ndarray:
    """[N,2] (y, x) of the pixel farthest from the object boundary for every label (reference :1322-1355)."""
    from ._label_image_ops import blockwise_distance_transform, find_outer_boundaries, label_regions
    interior = ~find_outer_boundaries(segmentation)
    if avoid_image_border:
        interior[0, :] = interior[-1, :] = False
        interior[:, 0] = interior[:, -1] = False
    distances = blockwise_distance_transform(interior, halo=(16, 16), block_shape=(512, 512))
    centers = []
    for seg_id, bb, _ in label_regions(segmentation):
        dist = np.where(segmentation[bb] == seg_id, distances[bb], 0)
        cy, cx = np.unravel_index(np.argmax(dist), dist.shape)           # first maximum in raster order
        centers.append((cy + bb[0].start, cx + bb[1].start))
    return np.array(centers)


def _derive_point_prompts(foreground: np.ndarray, center_distances: np.ndarray, boundary_distances: np.ndarray,
                          foreground_threshold: float = 0.5, center_distance_threshold: float = 0.5,
                          boundary_distance_threshold: float = 0.5):
    """One positive point per connected component of {foreground, close to a centre, far from a boundary}
    (reference :1358-1379); ``None`` when there is no component."""
    seeds = (center_distances < center_distance_threshold) & (boundary_distances < boundary_distance_threshold)
    seeds[foreground < foreground_threshold] = False
    components = util._label_equal_value_components(seeds.astype("uint32"))
    prompts = _get_centers(components)
    if len(prompts) == 0:
        return None
    return {"points": prompts[:, None, ::-1], "point_labels": np.ones((len(prompts), 1))}


def _derive_point_prompts_device(foreground, center_distances, boundary_distances, foreground_threshold: float = 0.5,
                                 center_distance_threshold: float = 0.5, boundary_distance_threshold: float = 0.5):
    """``_derive_point_prompts`` on the device (``ops.seed_centers``, csrc/labelprops.hip): the same keywords, the same return value,
    integer for integer.  The maps are device tensors or numpy arrays (uploaded); only the number of components and their centres come
    back.  Where the reference's blockwise distance transform is undefined (a component that fills a whole 544 x 544 window) the host
    function answers."""
    from . import _lib, ops
    dev = next((m.device for m in (foreground, center_distances, boundary_distances) if torch.is_tensor(m)), None)
    dev = _lib.require_gpu() if dev is None else dev
    # float32 maps only (ops.seed_centers refuses anything else): another type would compare differently from the host function
    maps = [m.contiguous() if torch.is_tensor(m) else torch.from_numpy(np.ascontiguousarray(m)).to(dev)
            for m in (foreground, center_distances, boundary_distances)]
    found = ops.seed_centers(*maps, foreground_threshold=foreground_threshold, center_distance_threshold=center_distance_threshold,
                             boundary_distance_threshold=boundary_distance_threshold)
    if found.undefined:
        return _derive_point_prompts(*(m.cpu().numpy() for m in maps), foreground_threshold=foreground_threshold,
                                     center_distance_threshold=center_distance_threshold,
                                     boundary_distance_threshold=boundary_distance_threshold)
    if found.n == 0:
        return None
    prompts = found.centers.cpu().numpy().astype(np.int64)
    return {"points": prompts[:, None, ::-1], "point_labels": np.ones((len(prompts), 1))}


def _derive_box_prompts(predictions, box_extension: float):
    """Boxes around the masks of a first round of predictions, grown by ``box_extension`` (reference :1382-1391; the
    clipping against ``shape[0]`` / ``shape[1]`` is the reference's)."""
    shape = predictions[0]["segmentation"].shape
    prompts = [[max(x - w * box_extension, 0), max(y - h * box_extension, 0),
                min(x + (1 + box_extension) * w, shape[0]), min(y + (1 + box_extension) * h, shape[1])]
               for (x, y, w, h) in (pred["bbox"] for pred in predictions)]
    return {"boxes": np.array(prompts)}


def _gaussian(x: np.ndarray, sigma: float) -> np.ndarray:
    from scipy import ndimage
    return ndimage.gaussian_filter(np.asarray(x, dtype=np.float32), sigma, mode="mirror", truncate=3.0)


def seeded_watershed(heights: np.ndarray, markers: np.ndarray, mask: Optional[np.ndarray] = None) -> np.ndarray:
    """``skimage.segmentation.watershed(heights, markers=markers, mask=mask)`` (connectivity 1, no compactness) through the
    library's host priority flood (msam_host_seeded_watershed)."""
    import ctypes as C
    from . import _lib
    h = np.ascontiguousarray(heights, dtype=np.float32)
    m = np.ascontiguousarray(markers, dtype=np.int32)
    assert h.ndim == 2 and m.shape == h.shape
    mk = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    out = np.empty(h.shape, dtype=np.int32)
    _lib.check(_lib.load().msam_host_seeded_watershed(h.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p),
                                                      None if mk is None else mk.ctypes.data_as(C.c_void_p), h.shape[0], h.shape[1],
                                                      out.ctypes.data_as(C.c_void_p)), "msam_host_seeded_watershed")
    return out


def watershed_from_center_and_boundary_distances(center_distances, boundary_distances, foreground_map,
                                                 center_distance_threshold: float = 0.5, boundary_distance_threshold: float = 0.5,
                                                 foreground_threshold: float = 0.5, distance_smoothing: float = 1.6,
                                                 min_size: int = 0) -> np.ndarray:
    """``torch_em.util.segmentation.watershed_from_center_and_boundary_distances`` (called at reference :1131-1140), restated:
    smooth both distance maps, seeds where both are below their thresholds inside the foreground, label the seeds (8-connected,
    raster order), flood the smoothed boundary distances from them inside the foreground mask, drop objects below ``min_size``
    and renumber consecutively."""
    from scipy import ndimage
    center = _gaussian(center_distances, distance_smoothing) if distance_smoothing > 0 else np.asarray(center_distances, np.float32)
    boundary = _gaussian(boundary_distances, distance_smoothing) if distance_smoothing > 0 else np.asarray(boundary_distances, np.float32)
    fg = np.asarray(foreground_map) > foreground_threshold
    seeds = (center < center_distance_threshold) & (boundary < boundary_distance_threshold)
    seeds[~fg] = False
    markers, _ = ndimage.label(seeds, structure=np.ones((3, 3), dtype=bool))
    seg = seeded_watershed(boundary, markers, fg).astype(np.uint32)
    if min_size > 0:
        ids, sizes = np.unique(seg, return_counts=True)
        seg[np.isin(seg, ids[sizes < min_size])] = 0
        keep = np.unique(seg)
        keep = keep[keep != 0]
        lut = np.zeros(int(seg.max()) + 1, dtype=np.uint32)
        lut[keep] = np.arange(1, len(keep) + 1, dtype=np.uint32)
        seg = lut[seg]
    return seg


class InstanceSegmentationWithDecoder:
    """State handling of the reference's decoder-based segmenters (:953-1207): ``initialize`` runs ``decoder(embeddings,
    input_shape, original_shape) -> [1, 3, H, W]`` (foreground, centre distances, boundary distances) on the predictor's
    embedding of the image.  The decoder is any callable with that signature - the reference's ``DecoderAdapter`` around
    ``torch_em.model.UNETR`` (:688-828) is not part of this build (torch_em is not vendored in the reference).

    ``generate`` is the reference's seeded watershed (:1083-1168) on the host, as in the reference (restated over scipy and the
    library's priority flood: vigra / scikit-image / torch_em are absent); ``AutomaticPromptGenerator`` below derives point prompts
    from the same state instead."""

    def __init__(self, predictor: SamPredictor, decoder) -> None:
        self._predictor = predictor
        self._decoder = decoder
        self._foreground = self._center_distances = self._boundary_distances = None
        self._device_maps = None                # the decoder output [3, H, W] where it was computed, when that is the device
        self._is_initialized = False

    @property
    def is_initialized(self):
        return self._is_initialized

    @torch.no_grad()
    def initialize(self, image: np.ndarray, image_embeddings=None, i: Optional[int] = None, verbose: bool = False,
                   pbar_init: Optional[callable] = None, pbar_update: Optional[callable] = None, ndim: int = 2) -> None:
        _, pbar_init, pbar_update, pbar_close = util.handle_pbar(verbose, pbar_init, pbar_update)
        pbar_init(1, "Initialize instance segmentation with decoder")
        if image_embeddings is None:
            image_embeddings = util.precompute_image_embeddings(self._predictor, image, ndim=ndim, verbose=verbose)
        self._predictor = util.set_precomputed(self._predictor, image_embeddings, i=i)
        output = self._decoder(self._predictor.features, tuple(self._predictor.input_size),
                               tuple(self._predictor.original_size))
        device_maps = output.float().squeeze(0).contiguous() if torch.is_tensor(output) and output.is_cuda else None
        output = (output.float().cpu().numpy() if torch.is_tensor(output) else np.asarray(output)).squeeze(0)
        assert output.shape[0] == 3, f"{output.shape}"
        self._device_maps = device_maps
        pbar_update(1)
        pbar_close()
        self._foreground, self._center_distances, self._boundary_distances = output[0], output[1], output[2]
        self._i = i
        self._is_initialized = True

    def _to_masks(self, segmentation: np.ndarray, output_mode: str):
        """Label image -> list of mask records (reference :1040-1081, 2-d)."""
        from ._label_image_ops import label_regions
        if output_mode != "binary_mask":
            raise ValueError(f"Output mode {output_mode} is not supported. Choose one of 'instance_segmentation', 'binary_masks'")
        assert segmentation.ndim == 2
        shape = segmentation.shape
        crop_box = [0, shape[1], 0, shape[0]]
        return [{"segmentation": segmentation == seg_id, "area": area,
                 "bbox": [bb[1].start, bb[1].stop - bb[1].start, bb[0].start, bb[0].stop - bb[0].start],    # [x0, w, y0, h]
                 "crop_box": crop_box, "seg_id": seg_id} for seg_id, bb, area in label_regions(segmentation)]

    def generate(self, center_distance_threshold: float = 0.5, boundary_distance_threshold: float = 0.5,
                 foreground_threshold: float = 0.5, foreground_smoothing: float = 1.0, distance_smoothing: float = 1.6,
                 min_size: int = 0, output_mode: str = "instance_segmentation", tile_shape=None, halo=None, n_threads=None,
                 optimize_memory: bool = False, segmentation=None):
        """Reference :1083-1168 (``tile_shape`` / ``halo`` / ``n_threads`` / ``optimize_memory`` only parallelise the reference's host
        post-processing and are accepted and ignored): Gaussian smoothing of the three maps, seeds = connected components of
        {centre distance < t, boundary distance < t, foreground > t}, seeded watershed of the smoothed boundary distances inside
        the foreground (``watershed_from_center_and_boundary_distances``), size filter.  Host arithmetic as in the reference -
        restated over scipy + the library's priority flood because vigra / scikit-image / torch_em are absent: the Gaussian is
        vigra's (window 3 sigma, mirrored border) through ``scipy.ndimage.gaussian_filter(truncate=3, mode="mirror")``, the seeds are
        8-connected (scikit-image's ``label`` default), the flood is scikit-image's published algorithm (csrc/watershed.hip).
        PARITY UNPINNED against those libraries."""
        if not self.is_initialized:
            raise RuntimeError("InstanceSegmentationWithDecoder has not been initialized. Call initialize first.")
        seg = watershed_from_center_and_boundary_distances(
            self._center_distances, self._boundary_distances,
            _gaussian(self._foreground, foreground_smoothing) if foreground_smoothing > 0 else self._foreground,
            center_distance_threshold, boundary_distance_threshold, foreground_threshold, distance_smoothing, min_size)
        if segmentation is not None:
            segmentation[:] = seg
            seg = segmentation
        if output_mode == "instance_segmentation":
            return seg
        return self._to_masks(seg, output_mode)

    def get_state(self) -> Dict[str, Any]:
        if not self.is_initialized:
            raise RuntimeError("The state has not been computed yet. Call initialize first.")
        return {"foreground": self._foreground, "center_distances": self._center_distances,
                "boundary_distances": self._boundary_distances}

    def set_state(self, state: Dict[str, Any]) -> None:
        self._foreground = state["foreground"]
        self._center_distances = state["center_distances"]
        self._boundary_distances = state["boundary_distances"]
        self._device_maps = None
        self._is_initialized = True

    def clear_state(self):
        self._foreground = self._center_distances = self._boundary_distances = None
        self._device_maps = None
        self._is_initialized = False


class TiledInstanceSegmentationWithDecoder(InstanceSegmentationWithDecoder):
    """The same on tiled embeddings (reference :1210-1319): the decoder runs per tile (outer block), the inner blocks of
    its three maps are written into full-image maps."""

    @torch.no_grad()
    def initialize(self, image: np.ndarray, image_embeddings=None, i: Optional[int] = None, tile_shape=None, halo=None,
                   verbose: bool = False, pbar_init: Optional[callable] = None, pbar_update: Optional[callable] = None,
                   batch_size: int = 1, mask=None) -> None:
        from .tiling import Blocking
        original_size = image.shape[:2]
        self._image_embeddings, tile_shape, halo, tiles_in_mask = _process_tiled_embeddings(
            self._predictor, image, image_embeddings, tile_shape, halo, verbose=verbose, batch_size=batch_size, mask=mask, i=i)
        tiling = Blocking([0, 0], original_size, tile_shape)
        _, pbar_init, pbar_update, pbar_close = util.handle_pbar(verbose, pbar_init, pbar_update)
        maps = np.zeros((3,) + tuple(original_size), dtype="float32")
        device_maps, on_device = None, True     # the same stitching on the device, as long as every tile's output arrives there
        tile_ids = list(range(tiling.number_of_blocks)) if tiles_in_mask is None else list(tiles_in_mask)
        pbar_init(len(tile_ids), "Initialize tiled instance segmentation with decoder" + ("" if tiles_in_mask is None else " and mask"))
        for tile_id in tile_ids:
            self._predictor = util.set_precomputed(self._predictor, self._image_embeddings, i=i, tile_id=tile_id)
            output = self._decoder(self._predictor.features, tuple(self._predictor.input_size),
                                   tuple(self._predictor.original_size))
            device_output = output.float().squeeze(0) if torch.is_tensor(output) and output.is_cuda else None
            output = (output.float().cpu().numpy() if torch.is_tensor(output) else np.asarray(output)).squeeze(0)
            assert output.shape[0] == 3
            block = tiling.get_block_with_halo(tile_id, halo=list(halo))
            local = tuple(slice(b, e) for b, e in zip(block.inner_block_local.begin, block.inner_block_local.end))
            inner = tuple(slice(b, e) for b, e in zip(block.inner_block.begin, block.inner_block.end))
            maps[(slice(None),) + inner] = output[(slice(None),) + local]
            on_device = on_device and device_output is not None
            if on_device:
                if device_maps is None:
                    device_maps = torch.zeros((3,) + tuple(original_size), dtype=torch.float32, device=device_output.device)
                device_maps[(slice(None),) + inner] = device_output[(slice(None),) + local]
            pbar_update(1)
        pbar_close()
        self._i = i
        self._foreground, self._center_distances, self._boundary_distances = maps[0], maps[1], maps[2]
        self._device_maps = device_maps if on_device else None
        self._is_initialized = True


class AutomaticPromptGenerator(InstanceSegmentationWithDecoder):
    """Instance segmentation from prompts derived from the decoder maps (reference :1394-1505): components of the
    thresholded maps -> one point per component -> ``inference.batched_inference`` on the HIP decoder ->
    ``util.apply_nms`` (device mask NMS) -> label image."""

    def generate(self, min_size: int = 25, center_distance_threshold: float = 0.5, boundary_distance_threshold: float = 0.5,
                 foreground_threshold: float = 0.5, multimasking: bool = False, batch_size: int = 32,
                 nms_threshold: float = 0.9, intersection_over_min: bool = False, output_mode: str = "instance_segmentation",
                 mask_threshold: Optional[Union[float, str]] = None, refine_with_box_prompts: bool = False,
                 prompt_function: Optional[callable] = None) -> Union[List[Dict[str, Any]], np.ndarray]:
        from .inference import batched_inference
        if not self.is_initialized:
            raise RuntimeError("AutomaticPromptGenerator has not been initialized. Call initialize first.")
        foreground = self._foreground
        device_maps = getattr(self, "_device_maps", None)
        if prompt_function is None and device_maps is not None:      # the decoder's own output is still on the device: derive there
            prompts = _derive_point_prompts_device(device_maps[0], device_maps[1], device_maps[2],
                                                   foreground_threshold=foreground_threshold,
                                                   center_distance_threshold=center_distance_threshold,
                                                   boundary_distance_threshold=boundary_distance_threshold)
        else:
            prompt_function = _derive_point_prompts if prompt_function is None else prompt_function
            prompts = prompt_function(foreground=foreground, center_distances=self._center_distances,
                                      boundary_distances=self._boundary_distances, foreground_threshold=foreground_threshold,
                                      center_distance_threshold=center_distance_threshold,
                                      boundary_distance_threshold=boundary_distance_threshold)
        if prompts is None:
            return np.zeros(foreground.shape, dtype="uint32") if output_mode == "instance_segmentation" else []

        def predict(prompts):
            return batched_inference(self._predictor, image=None, batch_size=batch_size, return_instance_segmentation=False,
                                     multimasking=multimasking, mask_threshold=mask_threshold, i=getattr(self, "_i", None),
                                     **prompts)
        predictions = predict(prompts)
        if refine_with_box_prompts:
            predictions = predict(_derive_box_prompts(predictions, box_extension=0.01))
        segmentation = util.apply_nms(predictions, min_size=min_size, nms_thresh=nms_threshold,
                                      intersection_over_min=intersection_over_min)
        if output_mode != "instance_segmentation":
            segmentation = self._to_masks(segmentation, output_mode)
        return segmentation


class TiledAutomaticPromptGenerator(TiledInstanceSegmentationWithDecoder):
    """``AutomaticPromptGenerator`` on tiled embeddings (reference :1508-1628): the prompts are derived on the stitched
    maps, every prompt is decoded on the tile that contains it (``inference.batched_tiled_inference``), the tile-local
    records meet in ``util.apply_nms`` through their ``global_bbox``."""

    def generate(self, min_size: int = 25, center_distance_threshold: float = 0.5, boundary_distance_threshold: float = 0.5,
                 foreground_threshold: float = 0.5, multimasking: bool = False, batch_size: int = 32,
                 nms_threshold: float = 0.9, intersection_over_min: bool = False, output_mode: str = "instance_segmentation",
                 mask_threshold: Optional[Union[float, str]] = None, refine_with_box_prompts: bool = False,
                 prompt_function: Optional[callable] = None, optimize_memory: bool = False):
        from .inference import batched_tiled_inference
        if not self.is_initialized:
            raise RuntimeError("TiledAutomaticPromptGenerator has not been initialized. Call initialize first.")
        if optimize_memory and (output_mode != "instance_segmentation" or refine_with_box_prompts):
            raise ValueError("Invalid settings")
        foreground = self._foreground
        device_maps = getattr(self, "_device_maps", None)
        if prompt_function is None and device_maps is not None:      # as in AutomaticPromptGenerator.generate, on the stitched maps
            prompts = _derive_point_prompts_device(device_maps[0], device_maps[1], device_maps[2],
                                                   foreground_threshold=foreground_threshold,
                                                   center_distance_threshold=center_distance_threshold,
                                                   boundary_distance_threshold=boundary_distance_threshold)
        else:
            prompt_function = _derive_point_prompts if prompt_function is None else prompt_function
            prompts = prompt_function(foreground, self._center_distances, self._boundary_distances,
                                      foreground_threshold=foreground_threshold,
                                      center_distance_threshold=center_distance_threshold,
                                      boundary_distance_threshold=boundary_distance_threshold)
        shape = foreground.shape
        if prompts is None:
            return np.zeros(shape, dtype="uint32") if output_mode == "instance_segmentation" else []
        if optimize_memory:
            prompts.update(dict(min_size=min_size, nms_thresh=nms_threshold, intersection_over_min=intersection_over_min))
        # (the reference does not forward mask_threshold here either)
        predictions = batched_tiled_inference(self._predictor, image=None, batch_size=batch_size,
                                              image_embeddings=self._image_embeddings, return_instance_segmentation=False,
                                              multimasking=multimasking, optimize_memory=optimize_memory,
                                              i=getattr(self, "_i", None), **prompts)
        if optimize_memory:
            return predictions
        if refine_with_box_prompts:
            raise NotImplementedError
        segmentation = util.apply_nms(predictions, shape=shape, min_size=min_size, nms_thresh=nms_threshold,
                                      intersection_over_min=intersection_over_min)
        if output_mode != "instance_segmentation":
            segmentation = self._to_masks(segmentation, output_mode)
        return segmentation

    def get_state(self):
        raise NotImplementedError

    def set_state(self, state):
        raise NotImplementedError


# ---- the decoder module itself (reference :688-870; models/unetr.py: torch_em's UNETR restated, widths read from the checkpoint)
from .models.unetr import DecoderAdapter, get_decoder, get_unetr  # noqa: E402,F401


def get_predictor_and_decoder(model_type: str, checkpoint_path=None, device=None, peft_kwargs: Optional[Dict] = None):
    """Reference ``get_predictor_and_decoder`` (:831-870): the predictor and the instance segmentation decoder of a checkpoint that
    holds both (``{"model_state", "decoder_state"}``)."""
    predictor, state = util.get_sam_model(model_type=model_type, checkpoint_path=checkpoint_path, device=device, return_state=True,
                                          peft_kwargs=peft_kwargs)
    if "decoder_state" not in state:
        raise ValueError(f"The checkpoint at '{checkpoint_path}' or the chosen model '{model_type}' does not contain a decoder state")
    return predictor, get_decoder(predictor.model.image_encoder, state["decoder_state"], predictor.device)


def get_instance_segmentation_generator(predictor: SamPredictor, is_tiled: bool = False, decoder=None,
                                        segmentation_mode: Optional[str] = None, **kwargs):
    """Factory with the reference's signature and mode resolution (:1631-1690): ``amg`` without a decoder, ``ais`` (the reference's
    ``DEFAULT_SEGMENTATION_MODE_WITH_DECODER`` :44) with one."""
    if segmentation_mode is None:
        segmentation_mode = "amg" if decoder is None else DEFAULT_SEGMENTATION_MODE_WITH_DECODER
    mode = segmentation_mode.lower()
    if mode == "amg":
        return (TiledAutomaticMaskGenerator if is_tiled else AutomaticMaskGenerator)(predictor, **kwargs)
    if mode == "ais":
        assert decoder is not None
        return (TiledInstanceSegmentationWithDecoder if is_tiled else InstanceSegmentationWithDecoder)(predictor, decoder, **kwargs)
    if mode == "apg":
        assert decoder is not None
        return (TiledAutomaticPromptGenerator if is_tiled else AutomaticPromptGenerator)(predictor, decoder, **kwargs)
    raise ValueError(f"Invalid segmentation_mode: {segmentation_mode}. Choose one of 'amg', 'ais', or 'apg'.")
