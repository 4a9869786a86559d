"""micro_sam.util's hot-path surface on the MI355X core: ``get_sam_model``, ``precompute_image_embeddings``,
``set_precomputed``, ``_to_image``, ``mask_data_to_segmentation`` (reference: micro_sam/util.py:318-476,618-681,
902-1018,1133-1258,1773-1848).  Same names, argument meaning and error behaviour; what is not provided this round
raises ``NotImplementedError`` naming the missing piece instead of silently differing.  The on-disk embedding cache
(``save_path``) is a zarr v2 container written / read by ``zarr_store``.
"""
from __future__ import annotations

import os
import warnings
from collections import OrderedDict
from typing import Any, Callable, Dict, List, Optional, Tuple, Union

import numpy as np
import torch

from . import _lib, modeling
from .predictor import SamPredictor

ImageEmbeddings = Dict[str, Any]
_DEFAULT_MODEL = "vit_b"


def get_device(device: Optional[Union[str, torch.device]] = None) -> Union[str, torch.device]:
    """Reference util.py:204-231, restricted to what this build can run on: an AMD GPU."""
    if device is None or device == "auto":
        if not torch.cuda.is_available():
            raise RuntimeError("micro_sam_amd requires a GPU (PyTorch-ROCm 'cuda' device); none is available.")
        return "cuda"
    dev_type = torch.device(device).type if not isinstance(device, str) else device.lower().split(":")[0]
    if dev_type != "cuda":
        raise RuntimeError(f"Unsupported device: {device}. micro_sam_amd only runs on 'cuda' (ROCm) devices.")
    if not torch.cuda.is_available():
        raise RuntimeError("PyTorch CUDA (ROCm) backend is not available.")
    return device


def _compute_hash(path: str) -> str:
    import xxhash
    h = xxhash.xxh128()
    with open(path, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 20), b""):
            h.update(chunk)
    return f"xxh128:{h.hexdigest()}"


def _load_checkpoint(checkpoint_path: str):
    """torch_em style ({'model_state', 'decoder_state'}, 'sam.' prefix) or plain SAM state dict (util.py:273-290)."""
    try:
        state = torch.load(checkpoint_path, map_location="cpu", weights_only=True)      # plain tensors: no code execution
    except Exception:
        # torch_em checkpoints pickle optimizer / trainer objects next to the tensors: unpickling them runs code from the
        # file - only load checkpoints you trust (same as the reference, micro_sam/util.py:277)
        state = torch.load(checkpoint_path, map_location="cpu", weights_only=False)
    if "model_state" in state:
        model_state = OrderedDict((k[len("sam."):] if k.startswith("sam.") else k, v)
                                  for k, v in state["model_state"].items())
    else:
        model_state = state
    return state, model_state


def _hash_state_dict(state_dict) -> str:
    """xxh128 over the sorted keys, shapes and bytes of a state dict: embedding caches computed with other weights of the
    same model type are detected (``_check_saved_embeddings`` compares ``predictor._hash``)."""
    import xxhash
    h = xxhash.xxh128()
    for k in sorted(state_dict):
        t = state_dict[k].detach().cpu().contiguous()
        h.update(k.encode()); h.update(str(tuple(t.shape)).encode()); h.update(str(t.dtype).encode())
        h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes() if t.numel() else b"")      # (reshape: 0-dim BatchNorm counters)
    return f"xxh128:{h.hexdigest()}"


def _validate_model_type(state) -> str:
    """micro_sam/models/build_sam.py:24-37."""
    if "image_encoder.patch_embed.proj.weight" in state:
        return {768: "vit_b", 1024: "vit_l", 1280: "vit_h"}[state["image_encoder.patch_embed.proj.weight"].shape[0]]
    return "vit_t"


def get_sam_model(model_type: str = _DEFAULT_MODEL, device: Optional[Union[str, torch.device]] = None,
                  checkpoint_path: Optional[Union[str, os.PathLike]] = None, return_sam: bool = False,
                  return_state: bool = False, peft_kwargs: Optional[Dict] = None, flexible_load_checkpoint: bool = False,
                  progress_bar_factory: Optional[Callable] = None, state_dict: Optional[Dict[str, torch.Tensor]] = None,
                  **model_kwargs):
    """Build the HIP-backed SAM and wrap it in a ``SamPredictor`` (reference util.py:318-476).

    ``state_dict`` (extension): an upstream-named state dict used instead of a checkpoint file - the build / GPU
    environments have no network, so the reference's pooch download of named models is not available; without
    ``checkpoint_path`` or ``state_dict`` this raises."""
    device = get_device(device)
    abbreviated = model_type[:5]
    if abbreviated not in ("vit_b", "vit_l", "vit_h", "vit_t"):
        raise ValueError(f"Invalid model_type: {abbreviated}. Expect one of ('vit_h', 'vit_b', 'vit_l', 'vit_t')")
    state, model_hash = None, "xxh128:synthetic"
    if checkpoint_path is not None:
        checkpoint_path = str(checkpoint_path)
        model_hash = _compute_hash(checkpoint_path)
        state, model_state = _load_checkpoint(checkpoint_path)
        provided = _validate_model_type(model_state)
        if abbreviated != provided:
            warnings.warn(f"'model_type' {model_type!r} does not match the checkpoint ({provided!r}); using {provided!r}.")
            model_type = abbreviated = provided
    elif state_dict is not None:
        model_state = state_dict
        model_hash = _hash_state_dict(state_dict)
    else:
        raise RuntimeError("micro_sam_amd.get_sam_model: no network access for model downloads - pass checkpoint_path "
                           "(a SAM / micro_sam checkpoint file) or state_dict.")
    if abbreviated == "vit_t" and peft_kwargs and isinstance(peft_kwargs, dict):
        raise ValueError("'micro-sam' does not support parameter efficient finetuning for 'mobile-sam'.")
    sam = modeling.sam_model_registry[abbreviated](**model_kwargs)
    if peft_kwargs and isinstance(peft_kwargs, dict):
        # PEFT surgery of the image encoder before the weights are loaded (reference util.py:441-450); LoRA / FacT / SSF
        # updates are merged into the encoder's operand copies at inference, an AdaptFormer branch runs as its own kernel
        # (models/peft_sam.py)
        from .models import peft_sam
        peft_kwargs = dict(peft_kwargs)
        peft_kwargs.pop("quantize", None)
        sam = peft_sam.PEFT_Sam(sam, **peft_kwargs).sam
    if flexible_load_checkpoint:
        own = sam.state_dict()
        model_state = {k: v for k, v in model_state.items() if k in own and own[k].shape == v.shape}
        sam.load_state_dict(model_state, strict=False)
    else:
        sam.load_state_dict(model_state)
    sam.to(device=device)
    predictor = SamPredictor(sam)
    predictor.model_type = abbreviated
    predictor._hash = model_hash
    predictor.model_name = model_type
    predictor.checkpoint_path = checkpoint_path
    if return_sam and return_state:
        return predictor, sam, state
    if return_sam:
        return predictor, sam
    if return_state:
        return predictor, state
    return predictor


# ------------------------------------------------------------------------------------------------ embeddings

def _to_image(image):
    """Any 2-d / HWC array -> uint8 RGB with per-channel min-max normalisation (reference util.py:618-651)."""
    input_ = image
    ndim = input_.ndim
    n_channels = 1 if ndim == 2 else input_.shape[-1]
    if ndim == 2 or (ndim == 3 and n_channels == 1):
        # grayscale: the three channels are copies of each other, so the per-channel arithmetic below gives three identical planes;
        # it is done once on the contiguous plane and replicated (numpy's reduction over the leading axes of an HWC array costs 30 ms
        # per 1024^2 tile, the plane 0.5 ms) - bit-identical to the general path
        plane = np.ascontiguousarray(input_.reshape(input_.shape[:2])).astype("float32")
        plane -= plane.min()
        plane /= (plane.max() + np.float32(1e-7))
        u8 = (plane * 255).astype("uint8")
        return np.ascontiguousarray(np.repeat(u8[..., None], 3, axis=-1))
    if ndim == 2:
        input_ = np.concatenate([input_[..., None]] * 3, axis=-1)
    elif ndim == 3 and n_channels == 1:
        input_ = np.concatenate([input_] * 3, axis=-1)
    elif ndim == 3 and n_channels == 2:
        input_ = np.concatenate([input_, np.zeros(input_.shape[:2] + (1,), dtype=input_.dtype)], axis=-1)
    elif ndim == 3 and n_channels == 3:
        pass
    elif ndim == 3 and n_channels > 3:
        warnings.warn(f"You provided an input with {n_channels} channels. Only the first three will be used.")
        input_ = input_[..., :3]
    else:
        raise ValueError(f"Invalid input dimensionality {ndim}. Expect either a 2D input (=grayscale image) "
                         "or a 3D input (= image with channels).")
    assert input_.ndim == 3 and input_.shape[-1] == 3
    input_ = input_.astype("float32")
    flat = input_.reshape(-1, 3)                       # (a reduction over axis 0 of [HW, 3] instead of axes (0, 1) of [H, W, 3])
    input_ -= flat.min(axis=0)[None, None]
    input_ /= (flat.max(axis=0)[None, None] + 1e-7)
    return np.array((input_ * 255).astype("uint8"))


@torch.no_grad()
def _compute_embeddings_batched(predictor, batched_images):
    """Reference util.py:654-681; normalisation + padding are fused into the encoder's uint8 patch gather."""
    predictor.reset_image()
    tensors, original_sizes, input_sizes = [], [], []
    for image in batched_images:
        resized = predictor.transform.apply_image(image)
        original_sizes.append(image.shape[:2])
        input_sizes.append(tuple(resized.shape[:2]))
        tensors.append(torch.as_tensor(np.ascontiguousarray(resized)))
    if len({t.shape for t in tensors}) != 1:
        raise ValueError("All images of a batch must have the same shape.")
    batch = torch.stack(tensors).to(predictor.device, non_blocking=True)
    features = predictor.model.image_encoder.forward_u8(batch)
    predictor.original_size = original_sizes[-1]
    predictor.input_size = input_sizes[-1]
    predictor.features = features[-1:]
    predictor.is_image_set = True
    return features, original_sizes, input_sizes


def _device_to_image_ok(raw_images) -> bool:
    """Raw tiles of one shape with a dtype the device kernels take (``_to_image`` and - when the long side is not the encoder's
    1024 - Pillow's resize run on the device, both bit-identical to the host functions)."""
    first = raw_images[0]
    if not isinstance(first, np.ndarray) or first.ndim not in (2, 3):
        return False
    if any((not isinstance(im, np.ndarray)) or im.shape != first.shape or im.dtype != first.dtype for im in raw_images):
        return False
    return first.dtype.kind in "uif" and first.dtype.itemsize <= 4 and min(first.shape[:2]) >= 1


def _upload_raw_tiles(predictor, raw_images) -> torch.Tensor:
    """Host tiles -> one device tensor [B,H,W(,C)] (uint8 as is, anything else as float32) through a cached pinned staging
    buffer and an asynchronous copy: 1 MiB per uint8 1024^2 tile crosses PCIe instead of the 3 MiB RGB copy."""
    batch = np.stack(raw_images)
    if batch.dtype != np.uint8:
        batch = batch.astype(np.float32)
    # one grow-only page-locked buffer per element type, viewed at the batch's shape: the tiles of one tiled image come in several
    # shapes (border tiles), and page-locking a fresh buffer per shape cost 9 ms per batch (84 of 161 ms of a 2048^2 slice)
    # (two buffers in turn: the copy is queued on the compute stream behind the previous batch's kernels, and waiting for the upload
    # before last instead of the last one keeps the host one batch ahead of the device)
    src = torch.from_numpy(batch)
    ring = getattr(predictor, "_pin", None)
    if ring is None:
        ring = predictor._pin = {"slots": [None, None], "next": 0}
    k = ring["next"]
    ring["next"] = k ^ 1
    pin = ring["slots"][k]
    if pin is not None:
        pin[2].synchronize()                              # the upload out of this buffer (two batches ago) has completed
    if pin is None or pin[0] != batch.dtype.str or pin[1].numel() < src.numel():
        pin = (batch.dtype.str, torch.empty(max(src.numel(), 1 << 22), dtype=src.dtype).pin_memory(), torch.cuda.Event())
        ring["slots"][k] = pin
    view = pin[1][: src.numel()].view(src.shape)
    view.copy_(src)
    dev = view.to(predictor.device, non_blocking=True)
    pin[2].record()
    return dev


def to_image_device(raw: torch.Tensor) -> torch.Tensor:
    """``_to_image`` on the device for a raw tile [H,W] / [H,W,C] already in HBM -> uint8 [H,W,3] (bit-identical)."""
    from . import ops
    if raw.dim() == 3 and raw.shape[-1] > 3:
        warnings.warn(f"You provided an input with {raw.shape[-1]} channels. Only the first three will be used.")
    return ops.to_image(raw)


@torch.no_grad()
def _compute_embeddings_batched_raw(predictor, raw_images):
    """``_compute_embeddings_batched`` from RAW tiles: when no resize is needed the tiles are uploaded as they are and
    ``_to_image`` + ``Sam.preprocess`` run on the device; otherwise the host path (``_to_image``, PIL resize)."""
    on_gpu = str(predictor.device).startswith("cuda") and torch.cuda.is_available()
    if not (on_gpu and _device_to_image_ok(raw_images)):
        return _compute_embeddings_batched(predictor, [_to_image(im) for im in raw_images])
    predictor.reset_image()
    dev = _upload_raw_tiles(predictor, raw_images)
    return _embeddings_from_uploaded_raw(predictor, dev)


@torch.no_grad()
def _embeddings_from_uploaded_raw(predictor, dev: torch.Tensor):
    """The device part of ``_compute_embeddings_batched_raw``: raw tiles [B,H,W(,C)] already in HBM -> ``_to_image`` (+ the Pillow resize)
    + encoder, on the current stream."""
    batch = torch.stack([to_image_device(dev[b]) for b in range(dev.shape[0])])
    raw_images = [dev[b] for b in range(dev.shape[0])]
    size = tuple(dev.shape[1:3])
    input_size = tuple(predictor.transform.get_preprocess_shape(size[0], size[1], modeling.IMG_SIZE))
    if input_size != size:                   # ResizeLongestSide.apply_image: Pillow's bilinear resize, on the device
        from . import ops
        batch = ops.resize_bilinear_u8(batch, input_size[0], input_size[1])
    features = predictor.model.image_encoder.forward_u8(batch)
    predictor.original_size = size
    predictor.input_size = input_size
    predictor.features = features[-1:]
    predictor.is_image_set = True
    return features, [size] * len(raw_images), [input_size] * len(raw_images)


def handle_pbar(verbose, pbar_init, pbar_update):
    """Reference util.py:1098-1130."""
    if verbose and pbar_init is None:
        assert pbar_update is None
        from tqdm import tqdm
        pbar = tqdm()

        def pbar_init(total, description):
            pbar.total = total
            pbar.set_description(description)

        def pbar_update(update):
            pbar.update(update)

        def pbar_close():
            pbar.close()
    elif verbose and pbar_init is not None:
        assert pbar_update is not None
        pbar = None

        def pbar_close():
            pass
    else:
        pbar = None

        def noop(*args):
            pass

        pbar_init, pbar_update, pbar_close = noop, noop, noop
    return pbar, pbar_init, pbar_update, pbar_close


# -- on-disk cache: zarr v2 container (reference util.py:684-747 writers, :1038-1094 signature) ------------------

def _compute_data_signature(input_) -> str:
    """Reference util.py:1036-1038."""
    import hashlib
    return hashlib.sha1(np.asarray(input_).tobytes()).hexdigest()


def _get_embedding_signature(input_, predictor, tile_shape, halo, data_signature=None) -> Dict[str, Any]:
    """Reference util.py:1042-1055."""
    from . import __version__
    if data_signature is None:
        data_signature = _compute_data_signature(input_)
    return {
        "data_signature": data_signature,
        "tile_shape": tile_shape if tile_shape is None else [int(x) for x in tile_shape],
        "halo": halo if halo is None else [int(x) for x in halo],
        "model_type": predictor.model_type,
        "model_name": predictor.model_name,
        "micro_sam_version": __version__,
        "model_hash": getattr(predictor, "_hash", None),
    }


def _write_embedding_signature(f, input_, predictor, tile_shape, halo, input_size, original_size) -> None:
    """Reference util.py:1061-1065 (one .zattrs update instead of one per key)."""
    signature = _get_embedding_signature(input_, predictor, tile_shape, halo)
    signature.update({"input_size": input_size, "original_size": original_size})
    f.attrs.update(signature)


def _check_saved_embeddings(input_, predictor, f, save_path, tile_shape, halo) -> None:
    """Reference util.py:1068-1094: RuntimeError on a data / tiling / model_type mismatch, warning for the keys that
    were added later (version, model hash, model name)."""
    if "input_size" not in f.attrs:
        return
    attrs = f.attrs.asdict()
    signature = _get_embedding_signature(input_, predictor, tile_shape, halo)
    for key, val in signature.items():
        if key not in attrs or attrs[key] != val:
            if key in ("micro_sam_version", "model_hash", "model_name"):
                warnings.warn(f"The signature for {key} in embeddings file {save_path} has a mismatch: "
                              f"{attrs.get(key)} != {val}. This key was recently added, so your embeddings are likely "
                              "correct. But please recompute them if model predictions don't look as expected.")
            else:
                raise RuntimeError(f"Embeddings file {save_path} is invalid due to mismatch in {key}: "
                                   f"{attrs.get(key)} != {val}. Please recompute embeddings in a new file.")


def _write_batch(features, tile_ids, batched_embeddings, original_sizes, input_sizes, slices=None, n_slices=None) -> None:
    """Reference util.py:710-747: one dataset per tile ([1,256,64,64], or [Z,1,256,64,64] with chunk = one slice) with
    the ``original_size`` / ``input_size`` attrs.  One device -> host copy for the whole batch; the chunk files are
    written by a thread pool (file writes release the GIL)."""
    from concurrent import futures
    host = batched_embeddings.detach().float().cpu().numpy()
    datasets = {}
    if slices is not None:
        for k, tile_id in enumerate(tile_ids):      # dataset creation is not thread-safe: done up front
            name = str(tile_id)
            if name in datasets:
                continue
            if name in features:
                datasets[name] = features[name]
                continue
            ds = features.create_dataset(name, shape=(n_slices, 1) + host.shape[1:], dtype="float32",
                                         chunks=(1, 1) + host.shape[1:])
            ds.attrs.update({"original_size": original_sizes[k], "input_size": input_sizes[k]})
            datasets[name] = ds

    def _write_embed(k):
        name = str(tile_ids[k])
        if slices is None:
            ds = features.create_dataset(name, data=host[k:k + 1])
            ds.attrs.update({"original_size": original_sizes[k], "input_size": input_sizes[k]})
        else:
            datasets[name][slices[k]] = host[k:k + 1]

    n = len(tile_ids)
    if n == 1:
        _write_embed(0)
    elif n > 1:
        with futures.ThreadPoolExecutor(min(os.cpu_count() or 1, n, 16)) as tp:
            list(tp.map(_write_embed, range(n)))


def _compute_2d(input_, predictor, f, save_path, pbar_init, pbar_update, keep_on_device):
    """Reference util.py:907-934."""
    if save_path is not None and "input_size" in f.attrs:          # cached: load and set
        features = f["features"][:]
        image_embeddings = {"features": features, "input_size": tuple(f.attrs["input_size"]),
                            "original_size": tuple(f.attrs["original_size"])}
        set_precomputed(predictor, image_embeddings)
        if keep_on_device:
            image_embeddings["features"] = predictor.features
        return image_embeddings
    pbar_init(1, "Compute Image Embeddings 2D")
    predictor.reset_image()
    predictor.set_image(_to_image(input_))
    features = predictor.get_image_embedding()
    host = None
    if save_path is not None or not keep_on_device:
        host = features.cpu().numpy()
    pbar_update(1)
    if save_path is not None:
        f.create_dataset("features", data=host)
        _write_embedding_signature(f, input_, predictor, tile_shape=None, halo=None, input_size=predictor.input_size,
                                   original_size=predictor.original_size)
    return {"features": features if keep_on_device else host, "input_size": predictor.input_size,
            "original_size": predictor.original_size}


_PINNED: Dict[Any, torch.Tensor] = {}


def pinned_buffer(tag: str, shape, dtype: torch.dtype) -> torch.Tensor:
    """A cached page-locked host tensor of at least ``shape`` elements per (tag, dtype), viewed at ``shape`` (page-locking a fresh 64 MiB
    buffer costs tens of milliseconds: the double buffers of the pipelined loops are allocated once per process)."""
    n = int(np.prod(shape))
    key = (tag, dtype)
    stage = _PINNED.get(key)
    if stage is None or stage.numel() < n:
        stage = torch.empty(max(n, 1 << 20), dtype=dtype).pin_memory()
        _PINNED[key] = stage
    return stage[:n].view(tuple(shape))


def fetch_to_host(t: torch.Tensor, out: Optional[np.ndarray] = None, tag: str = "") -> np.ndarray:
    """Device tensor -> host array through a cached page-locked staging buffer (one per (tag, dtype), grown on demand): a DMA at PCIe
    speed + one host memcpy instead of a pageable copy (4 MiB label images / embeddings: ~0.5 ms instead of 1.2 - 2 ms).  Returns
    ``out`` (filled) or a fresh array; synchronises the current stream."""
    t = t.contiguous()
    if not t.is_cuda:                           # (host tensors of the CPU-side tests: nothing to stage)
        a = t.numpy()
        if out is None:
            return a.copy()
        np.copyto(out, a)
        return out
    key = (tag, t.dtype)
    stage = _PINNED.get(key)
    if stage is None or stage.numel() < t.numel():
        stage = torch.empty(max(t.numel(), 1 << 20), dtype=t.dtype).pin_memory()
        _PINNED[key] = stage
    view = stage[: t.numel()].view(t.shape)
    view.copy_(t, non_blocking=True)
    torch.cuda.current_stream(t.device).synchronize()
    if out is None:
        return view.numpy().copy()
    np.copyto(out, view.numpy())
    return out


def _compute_3d(input_, predictor, f, save_path, lazy_loading, pbar_init, pbar_update, batch_size, keep_on_device):
    """Reference util.py:950-1018, including the resume of a partially written container (slices whose chunk is all
    zero are recomputed)."""
    if save_path is not None and "input_size" in f.attrs:
        features = f["features"] if lazy_loading else f["features"][:]
        return {"features": features, "input_size": tuple(f.attrs["input_size"]),
                "original_size": tuple(f.attrs["original_size"])}
    n_slices = input_.shape[0]
    save_features = save_path is not None
    partial_features = False
    ds = None
    if save_features:
        shape = (n_slices, 1, modeling.PROMPT_DIM, modeling.GRID, modeling.GRID)
        chunks = (1,) + shape[1:]
        if "features" in f:
            partial_features = True
            ds = f["features"]
            if ds.shape != shape or ds.chunks != chunks:
                raise RuntimeError("Invalid partial features")
        else:
            ds = f.create_dataset("features", shape=shape, chunks=chunks, dtype="float32")
    pbar_init(n_slices, "Compute Image Embeddings 3D")
    features = []
    input_sizes = original_sizes = None
    # in-memory host result (the reference's contract): every batch goes to the host on a copy stream through a page-locked double
    # buffer WHILE the encoder works on the next batch, and the host fills (page-faults) the result array underneath as well
    stream_out = (not save_features and not keep_on_device and str(predictor.device).startswith("cuda") and torch.cuda.is_available())
    host_features, copy_stream, pins, pending = None, None, [None, None], None

    def drain(p):
        z0, z1, slot, ev = p
        ev.synchronize()
        np.copyto(host_features[z0:z1, 0], pins[slot][: z1 - z0].numpy())
    for bi, z_start in enumerate(range(0, n_slices, batch_size)):
        z_stop = min(z_start + batch_size, n_slices)
        zs = [z for z in range(z_start, z_stop)
              if not (partial_features and ds.chunk_initialized((z, 0, 0, 0, 0)) and np.count_nonzero(ds[z]) != 0)]
        if zs:
            emb, original_sizes, input_sizes = _compute_embeddings_batched_raw(predictor, [np.asarray(input_[z]) for z in zs])
            if save_features:
                host = emb.cpu().numpy()
                for k, z in enumerate(zs):
                    ds[z] = host[k:k + 1]
            else:
                features.append(emb.unsqueeze(1))          # [b,1,256,64,64]
                if stream_out and emb.is_cuda:
                    if host_features is None:
                        host_features = np.empty((n_slices, 1) + tuple(emb.shape[1:]), dtype=np.float32)
                        copy_stream = torch.cuda.Stream(device=emb.device)
                    slot = bi & 1
                    if pins[slot] is None:
                        pins[slot] = pinned_buffer(f"emb3d{slot}", (batch_size,) + tuple(emb.shape[1:]), torch.float32)
                    copy_stream.wait_stream(torch.cuda.current_stream(emb.device))
                    with torch.cuda.stream(copy_stream):
                        pins[slot][: len(zs)].copy_(emb, non_blocking=True)
                        ev = torch.cuda.Event()
                        ev.record(copy_stream)
                    emb.record_stream(copy_stream)
                    if pending is not None:
                        drain(pending)
                    pending = (z_start, z_stop, slot, ev)
        pbar_update(z_stop - z_start)
    if pending is not None:
        drain(pending)
    if input_sizes is None:          # every slice was already on disk: sizes from the data (what the encoder would report)
        image = _to_image(input_[n_slices - 1])
        original_sizes = [image.shape[:2]]
        input_sizes = [tuple(predictor.transform.get_preprocess_shape(image.shape[0], image.shape[1], 1024))]
    if save_features:
        _write_embedding_signature(f, input_, predictor, tile_shape=None, halo=None, input_size=input_sizes[-1],
                                   original_size=original_sizes[-1])
        features = ds if lazy_loading else ds[:]
    else:
        dev_features = torch.cat(features)
        features = dev_features
        if not keep_on_device:
            # the reference's in-memory result is a host array (util.py:1011-1013); it is filled batch by batch through a page-locked
            # staging buffer.  The returned dict holds exactly the reference's keys.  The device copy (<= 4 GiB) is remembered OUTSIDE
            # the dict, weakly keyed by the host array (_device_shadow): set_precomputed takes slice i from it instead of uploading
            # the 4 MiB it has just downloaded - only while the host array is still that object, at that address, with those values.
            if host_features is not None:
                features = host_features                      # filled batch by batch above
            else:
                features = np.empty(tuple(dev_features.shape), dtype=np.float32)
                step = max(1, batch_size)
                for z0 in range(0, n_slices, step):
                    fetch_to_host(dev_features[z0:z0 + step], out=features[z0:z0 + step], tag="emb")
            if dev_features.numel() * 4 <= (4 << 30):
                _remember_device_shadow(features, dev_features)
            return {"features": features, "input_size": input_sizes[-1], "original_size": original_sizes[-1]}
    return {"features": features, "input_size": input_sizes[-1], "original_size": original_sizes[-1]}


# host embedding array -> the device tensor it was downloaded from (the shadow is no dict entry, dies with the host array, and is
# used only after a check that the caller has not edited / replaced the slice it is asked for)
_DEVICE_SHADOWS: Dict[int, tuple] = {}


def _slice_digest(host: np.ndarray, i: Optional[int]) -> int:
    """64-bit digest of the WHOLE slice (xxh3: ~0.4 ms per 4 MiB slice; ADVICE r4: a strided sample of 256 values saw one point per channel,
    all in the first spatial rows, so zeroing half of every channel went unnoticed)."""
    sel = np.ascontiguousarray(host if i is None else host[i])
    try:
        import xxhash
        return xxhash.xxh3_64_intdigest(memoryview(sel).cast("B"))
    except ImportError:                                  # pragma: no cover - xxhash ships with the image
        import zlib
        return zlib.crc32(memoryview(sel).cast("B"))


def _remember_device_shadow(host: np.ndarray, dev: torch.Tensor) -> None:
    import weakref
    key = id(host)
    n = host.shape[0] if host.ndim == 5 else 1
    samples = [_slice_digest(host, z if host.ndim == 5 else None) for z in range(n)]
    _DEVICE_SHADOWS[key] = (weakref.ref(host, lambda _r, k=key: _DEVICE_SHADOWS.pop(k, None)), host.ctypes.data, tuple(host.shape),
                            samples, dev)


def _device_shadow(host, i: Optional[int]) -> Optional[torch.Tensor]:
    """The device copy of slice ``i`` of a host embedding array this process computed, or None (unknown array, other address /
    shape, or a slice whose digest differs from what was downloaded: the caller masked, reloaded or replaced ANY of its values)."""
    if not isinstance(host, np.ndarray):
        return None
    hit = _DEVICE_SHADOWS.get(id(host))
    if hit is None or hit[0]() is not host or hit[1] != host.ctypes.data or hit[2] != tuple(host.shape):
        return None
    z = 0 if (i is None or host.ndim != 5) else int(i)
    if _slice_digest(host, i if host.ndim == 5 else None) != hit[3][z]:
        return None
    return hit[4][:] if i is None else hit[4][i]


def load_image_data(path: Union[str, os.PathLike], key: Optional[str] = None, lazy_loading: bool = False):
    """Reference ``util.load_image_data`` (util.py:1334-1353): image data of a file, or of dataset / pattern ``key`` inside a container
    or folder.  The reference reads through imageio and ``elf.io.open_file``; neither is vendored, so the readers here are the ones this
    environment has, each optional: ``.npy`` / ``.npz`` (numpy), image files through imageio when importable, else Pillow (a multi-page
    TIFF becomes a stack), zarr / n5-style directories through the package's own zarr reader (``lazy_loading`` keeps the array object),
    hdf5 through h5py when importable, and a folder with a glob pattern as ``key`` = the sorted images stacked (elf's image-stack
    wrapper).  Anything else raises with the reason."""
    path = os.fspath(path)
    ext = os.path.splitext(path)[1].lower()

    def read_image(p):
        if os.path.splitext(p)[1].lower() == ".npy":
            return np.load(p)
        try:
            import imageio.v3 as iio
            return np.asarray(iio.imread(p))
        except ImportError:
            pass
        from PIL import Image
        with Image.open(p) as im:
            n = getattr(im, "n_frames", 1)
            if n == 1:
                return np.asarray(im)
            frames = []
            for k in range(n):
                im.seek(k)
                frames.append(np.asarray(im))
            return np.stack(frames)
    if key is None:
        if os.path.isdir(path):
            raise ValueError(f"load_image_data: {path} is a folder / container: a key (dataset name or glob pattern) is needed")
        return read_image(path)
    if os.path.isdir(path) and any(ch in key for ch in "*?["):
        import glob as _glob
        files = sorted(_glob.glob(os.path.join(path, key)))
        if not files:
            raise ValueError(f"load_image_data: no file matches {key!r} in {path}")
        return np.stack([read_image(f) for f in files])
    if ext == ".npz":
        with np.load(path) as f:
            return f[key]
    if ext in (".h5", ".hdf5", ".hdf"):
        try:
            import h5py
        except ImportError as exc:
            raise RuntimeError("load_image_data: reading hdf5 needs h5py, which is not installed here") from exc
        if lazy_loading:                          # the dataset handle is only valid while its file is open: the file stays open (as the
            return h5py.File(path, "r")[key]      # reference's lazy path does; the handle keeps the file object alive) - ADVICE r5
        with h5py.File(path, "r") as f:
            return f[key][:]
    if os.path.isdir(path):                       # zarr (v2 / v3) directory store
        from . import zarr_store
        arr = zarr_store.open(path, mode="r")[key]
        return arr if lazy_loading else arr[:]
    raise ValueError(f"load_image_data: do not know how to read {key!r} from {path}")


def _get_tiles_in_mask(mask, tiling, halo, z=None):
    """Reference util.py:748-762: ids of the tiles whose OUTER block contains mask foreground."""
    tiles = []
    for tile_id in range(tiling.number_of_blocks):
        tile = tiling.get_block_with_halo(tile_id, list(halo))
        outer_tile = tuple(slice(beg, end) for beg, end in zip(tile.outer_block.begin, tile.outer_block.end))
        if z is not None:
            outer_tile = (z,) + outer_tile
        if np.asarray(mask[outer_tile]).astype("bool").sum() != 0:
            tiles.append(tile_id)
    return tiles


def _compute_tiled_features_2d(predictor, input_, tile_shape, halo, f, pbar_init, pbar_update, batch_size, mask):
    """Reference util.py:765-803.  The embeddings stay on the device in a ``tiling.TiledFeatures`` (the reference's
    in-memory zarr group); with a container ``f`` they are also written to its ``features`` group."""
    from .tiling import Blocking, TileArray, TiledFeatures
    tiling = Blocking([0, 0], input_.shape[:2], tile_shape)
    n_tiles = tiling.number_of_blocks
    features = TiledFeatures(input_.shape[:2], tile_shape, halo)
    group = None
    if f is not None:
        group = f.require_group("features")
        group.attrs.update({"shape": input_.shape[:2], "tile_shape": tile_shape, "halo": halo})
    n_batches = int(np.ceil(n_tiles / batch_size))
    if mask is None:
        tile_ids_for_batches = [range(b * batch_size, min((b + 1) * batch_size, n_tiles)) for b in range(n_batches)]
        pbar_init(n_tiles, "Compute Image Embeddings 2D tiled")
    else:
        tiles_in_mask = _get_tiles_in_mask(mask, tiling, halo)
        pbar_init(len(tiles_in_mask), "Compute Image Embeddings 2D tiled with mask")
        tile_ids_for_batches = np.array_split(tiles_in_mask, n_batches)
    for tile_ids in tile_ids_for_batches:
        tile_ids = [int(t) for t in tile_ids]
        if len(tile_ids) == 0:
            continue
        groups = {}
        for tile_id in tile_ids:       # the encoder batches tiles of one shape (border tiles of a mosaic are smaller)
            tile = tiling.get_block_with_halo(tile_id, list(halo))
            outer_tile = tuple(slice(beg, end) for beg, end in zip(tile.outer_block.begin, tile.outer_block.end))
            image = np.asarray(input_[outer_tile])               # raw tile: _to_image runs on the device when no resize is needed
            groups.setdefault(image.shape[:2], []).append((tile_id, image))
        for members in groups.values():
            emb, original_sizes, input_sizes = _compute_embeddings_batched_raw(predictor, [im for _, im in members])
            for k, (tile_id, _) in enumerate(members):
                features[tile_id] = TileArray(emb[k:k + 1], original_sizes[k], input_sizes[k])
            if group is not None:
                _write_batch(group, [t for t, _ in members], emb, original_sizes, input_sizes)
        pbar_update(len(tile_ids))
    if f is not None:
        _write_embedding_signature(f, input_, predictor, tile_shape, halo, input_size=None, original_size=None)
    if mask is not None:
        features.attrs["tiles_in_mask"] = tiles_in_mask
        if group is not None:
            group.attrs["tiles_in_mask"] = tiles_in_mask
    return features


def _compute_tiled_features_3d(predictor, input_, tile_shape, halo, f, pbar_init, pbar_update, batch_size, mask):
    """Reference util.py:859-905 (per-slice tiles batched by shape)."""
    from .tiling import Blocking, TileArray, TiledFeatures
    assert input_.ndim == 3
    shape = input_.shape[1:]
    tiling = Blocking([0, 0], shape, tile_shape)
    features = TiledFeatures(shape, tile_shape, halo)
    group = None
    if f is not None:
        group = f.require_group("features")
        group.attrs.update({"shape": shape, "tile_shape": tile_shape, "halo": halo})
    n_slices = input_.shape[0]
    tiles_in_mask_per_slice = None
    if mask is not None:
        tiles_in_mask_per_slice = {z: _get_tiles_in_mask(mask, tiling, halo, z=z) for z in range(n_slices)}
    work = [(z, t) for z in range(n_slices)
            for t in (range(tiling.number_of_blocks) if mask is None else tiles_in_mask_per_slice[z])]
    pbar_init(len(work), "Compute Image Embeddings 3D tiled" + ("" if mask is None else " masked"))
    store = {}
    for start in range(0, len(work), batch_size):
        chunk = work[start:start + batch_size]
        groups = {}
        for z, tile_id in chunk:
            tile = tiling.get_block_with_halo(tile_id, list(halo))
            outer_tile = (z,) + tuple(slice(beg, end) for beg, end in zip(tile.outer_block.begin, tile.outer_block.end))
            image = np.asarray(input_[outer_tile])
            groups.setdefault(image.shape[:2], []).append((z, tile_id, image))
        for members in groups.values():
            emb, original_sizes, input_sizes = _compute_embeddings_batched_raw(predictor, [im for _, _, im in members])
            for k, (z, tile_id, _) in enumerate(members):
                if tile_id not in store:
                    store[tile_id] = (torch.zeros((n_slices, 1) + tuple(emb.shape[1:]), dtype=emb.dtype, device=emb.device),
                                      original_sizes[k], input_sizes[k])
                store[tile_id][0][z, 0] = emb[k]
            if group is not None:
                _write_batch(group, [t for _, t, _ in members], emb, original_sizes, input_sizes,
                             slices=[z for z, _, _ in members], n_slices=n_slices)
        pbar_update(len(chunk))
    for tile_id, (data, original_size, input_size) in store.items():
        features[tile_id] = TileArray(data, original_size, input_size)
    if mask is not None:
        per_slice = {str(z): per_slice for z, per_slice in tiles_in_mask_per_slice.items()}
        features.attrs["tiles_in_mask"] = per_slice
        if group is not None:
            group.attrs["tiles_in_mask"] = per_slice
    if f is not None:
        _write_embedding_signature(f, input_, predictor, tile_shape, halo, input_size=None, original_size=None)
    return features


def precompute_image_embeddings(predictor: SamPredictor, input_: np.ndarray, save_path=None, lazy_loading: bool = False,
                                ndim: Optional[int] = None, tile_shape: Optional[Tuple[int, int]] = None,
                                halo: Optional[Tuple[int, int]] = None, verbose: bool = True, batch_size: int = 1,
                                mask=None, pbar_init: Optional[callable] = None, pbar_update: Optional[callable] = None,
                                keep_on_device: bool = False) -> ImageEmbeddings:
    """Reference util.py:1133-1212.  ``keep_on_device`` (extension): return the features as a device tensor instead of
    a host numpy array (``set_precomputed`` accepts both, as in the reference util.py:1248-1252).

    ``save_path``: zarr v2 container (``zarr_store``, same layout and signature attrs as the reference's cache): an
    existing container is validated against the input / tiling / model (``RuntimeError`` on a mismatch) and loaded,
    otherwise the embeddings are computed and written.  Freshly computed tiled embeddings (``tile_shape`` / ``halo``)
    are returned in a ``tiling.TiledFeatures`` container (device tensors) with the attrs of the reference's zarr group,
    cached ones as the container's ``features`` group; ``input_size`` / ``original_size`` are None for them
    (util.py:946,1034)."""
    from . import zarr_store
    ndim = input_.ndim if ndim is None else ndim
    if tile_shape is not None and halo is None:
        raise ValueError("To compute tiled embeddings the parameters tile_shape and halo have to be passed.")
    f = None
    if save_path is not None:
        save_path = os.fspath(save_path)
        existed = os.path.exists(save_path)
        f = zarr_store.open(save_path, mode="a")
        if existed:
            _check_saved_embeddings(input_, predictor, f, save_path, tile_shape, halo)
    _, pbar_init, pbar_update, pbar_close = handle_pbar(verbose, pbar_init, pbar_update)
    cached_tiled = f is not None and tile_shape is not None and "input_size" in f.attrs
    if ndim == 2 and tile_shape is None:
        embeddings = _compute_2d(input_, predictor, f, save_path, pbar_init, pbar_update, keep_on_device)
    elif ndim == 3 and tile_shape is None:
        embeddings = _compute_3d(input_, predictor, f, save_path, lazy_loading, pbar_init, pbar_update, batch_size,
                                 keep_on_device)
    elif ndim in (2, 3) and cached_tiled:          # reference util.py:937-943 / 1021-1027
        embeddings = {"features": f["features"], "input_size": f.attrs["input_size"],
                      "original_size": f.attrs["original_size"]}
    elif ndim == 2:
        features = _compute_tiled_features_2d(predictor, input_, tile_shape, halo, f, pbar_init, pbar_update, batch_size, mask)
        embeddings = {"features": features, "input_size": None, "original_size": None}
    elif ndim == 3:
        features = _compute_tiled_features_3d(predictor, input_, tile_shape, halo, f, pbar_init, pbar_update, batch_size, mask)
        embeddings = {"features": features, "input_size": None, "original_size": None}
    else:
        raise ValueError(f"Invalid dimesionality {input_.ndim}, expect 2 or 3 dim data.")
    pbar_close()
    return embeddings


def set_precomputed(predictor: SamPredictor, image_embeddings: ImageEmbeddings, i: Optional[int] = None,
                    tile_id: Optional[int] = None) -> SamPredictor:
    """Reference util.py:1215-1258."""
    if tile_id is not None:
        tile_features = image_embeddings["features"][str(tile_id)]
        tile_image_embeddings = {"features": tile_features, "input_size": tile_features.attrs["input_size"],
                                 "original_size": tile_features.attrs["original_size"]}
        return set_precomputed(predictor, tile_image_embeddings, i=i)
    device = predictor.device
    features = image_embeddings["features"]
    assert features.ndim in (4, 5), f"{features.ndim}"
    if features.ndim == 5 and i is None:
        raise ValueError("The data is 3D so an index i is needed.")
    elif features.ndim == 4 and i is not None:
        raise ValueError("The data is 2D so an index is not needed.")
    sel = _device_shadow(features, i)           # the device copy precompute_image_embeddings kept, if the host slice is unchanged
    if sel is None:
        sel = features[:] if i is None else features[i]
    predictor.features = sel.to(device) if torch.is_tensor(sel) else torch.from_numpy(np.asarray(sel[:])).to(device)
    predictor.original_size = tuple(image_embeddings["original_size"])
    predictor.input_size = tuple(image_embeddings["input_size"])
    predictor.is_image_set = True
    return predictor


def compute_iou(mask1: np.ndarray, mask2: np.ndarray) -> float:
    """Intersection over union of the pixels that equal 1 in two label images (reference util.py:1266-1280; host arithmetic
    in the reference as well - used between consecutive slices by the 3-d merging heuristics)."""
    m1, m2 = np.asarray(mask1) == 1, np.asarray(mask2) == 1
    overlap = np.logical_and(m1, m2).sum()
    union = np.logical_or(m1, m2).sum()
    return float(overlap) / (float(union) + 1e-7)


def _labels_on_device(segmentation) -> torch.Tensor:
    """A 2-d label image (numpy array or tensor) as a contiguous int32 tensor on the device the kernels run on."""
    ndim = segmentation.ndim
    if ndim != 2:
        raise ValueError(f"Only 2-d label images are supported, got an input with {ndim} dimensions.")
    device = _lib.require_gpu()
    if torch.is_tensor(segmentation):
        seg = segmentation
    else:
        seg = np.asarray(segmentation)
        if seg.dtype.kind not in "iub" or (seg.size and int(seg.max()) > 2 ** 31 - 1):
            raise ValueError(f"The label image must hold integer ids below 2^31, got {seg.dtype}.")
        seg = torch.from_numpy(np.ascontiguousarray(seg.astype(np.int32, copy=False)))
    return seg.to(device=device, dtype=torch.int32).contiguous()


def get_centers_and_bounding_boxes(segmentation, mode: str = "v") -> Tuple[Dict[int, tuple], Dict[int, tuple]]:
    """Reference util.py:1283-1331 on the device (``ops.label_props``, csrc/labelprops.hip): centre coordinates and bounding boxes
    (y0, x0, y1, x1, exclusive ends) of the objects of a 2-d label image, as two dicts keyed by object id.  mode "v": the object's
    pixel furthest from any inner boundary of the label image (always inside the object; among equally distant pixels the first in
    raster order), as tuples of ints; mode "p": the centroid, as tuples of floats.  ``segmentation``: a numpy array or a tensor; one
    device call and one copy back."""
    assert mode in ["p", "v"], "Choose either 'p' for regionprops centroids or 'v' for distance-based centers"
    from . import ops
    props = ops.label_props(_labels_on_device(segmentation), centers=mode == "v")
    n = int(props.ids.numel())
    if n == 0:
        return {}, {}
    third = props.center if mode == "v" else props.area[:, None]
    packed = torch.cat([props.ids[:, None].to(torch.int64), props.bbox.to(torch.int64), props.coord_sum, third.to(torch.int64)], dim=1).cpu().numpy()
    ids, bbox = packed[:, 0].tolist(), packed[:, 1:5].tolist()
    if mode == "v":
        centers = [(int(y), int(x)) for y, x in packed[:, 7:9].tolist()]
    else:
        mean = packed[:, 5:7].astype(np.float64) / packed[:, 7:8].astype(np.float64)
        centers = [(float(y), float(x)) for y, x in mean]
    center_coordinates = {int(i): c for i, c in zip(ids, centers)}
    bbox_coordinates = {int(i): tuple(int(v) for v in b) for i, b in zip(ids, bbox)}
    assert len(bbox_coordinates) == len(center_coordinates), f"{len(bbox_coordinates)}, {len(center_coordinates)}"
    return center_coordinates, bbox_coordinates


def segmentation_to_one_hot(segmentation, segmentation_ids=None) -> torch.Tensor:
    """Reference util.py:1356-1395: a label image -> float32 one-hot masks [N, 1, H, W].  Without ids N is the largest id and channel
    k holds id k + 1.  With ids: they are sorted, objects not selected are dropped, and - the reference relabels the remaining
    objects sequentially - the channels hold the selected ids that occur in the image in ascending order, followed by empty channels
    for those that do not.  A numpy input gives a CPU tensor as in the reference; a tensor stays on its device.  The comparison runs
    per channel against the id: no [max + 1, H, W] volume is built when ids are given."""
    seg = segmentation if torch.is_tensor(segmentation) else torch.from_numpy(np.ascontiguousarray(np.asarray(segmentation).astype(np.int64)))
    if segmentation_ids is None:
        n_ids = int(seg.max()) if seg.numel() else 0
        ids = torch.arange(1, n_ids + 1, device=seg.device, dtype=seg.dtype)
    else:
        msg = "No foreground objects were found."
        segmentation_ids = segmentation_ids.cpu().numpy() if torch.is_tensor(segmentation_ids) else np.asarray(segmentation_ids)
        if len(segmentation_ids) == 0 or 0 in segmentation_ids:
            raise RuntimeError(msg)
        n_ids = len(segmentation_ids)
        ids = torch.from_numpy(np.unique(segmentation_ids).astype(np.int64)).to(device=seg.device, dtype=seg.dtype)
    masks = seg[None] == ids.view(-1, *([1] * seg.dim()))
    if segmentation_ids is not None:
        masks = masks[masks.flatten(1).any(dim=1)]                       # relabel_sequential: only ids that occur keep a channel
        if masks.shape[0] < n_ids:
            masks = torch.cat([masks, torch.zeros((n_ids - masks.shape[0],) + tuple(seg.shape), dtype=torch.bool, device=seg.device)])
    return masks.to(torch.float32).unsqueeze(1)


# ------------------------------------------------------------------------------------------------ label image

def _block_major_keys(h: int, w: int, block: int = 512) -> np.ndarray:
    """Position of every pixel in block-major order (blocks of ``block`` x ``block`` in raster order, raster order inside a block):
    the order in which ``elf.parallel.label(block_shape=(512, 512))`` meets the pixels (csrc/common.h bm_key on the device)."""
    yy, xx = np.mgrid[0:h, 0:w]
    by, bx = yy // block, xx // block
    bh, bw = np.minimum(block, h - by * block), np.minimum(block, w - bx * block)
    return (by * block) * w + (bx * block) * bh + (yy % block) * bw + (xx % block)


def _label_equal_value_components(seg: np.ndarray) -> np.ndarray:
    """4-connected components of equal non-zero value, numbered the way the reference's ``elf.parallel.label(segmentation,
    block_shape=(512, 512))`` (util.py:1834-1838) numbers them: 512 x 512 blocks are labelled one by one in raster order with a
    running offset, united across block faces and made consecutive by first occurrence - a component's id is the rank of its first
    pixel in block-major order (plain raster order for images of up to 512 x 512).

    Components are found on the (2H-1)x(2W-1) pixel/link lattice with scipy's binary labelling, then renumbered."""
    from scipy import ndimage
    h, w = seg.shape
    lat = np.zeros((2 * h - 1, 2 * w - 1), dtype=bool)
    fg = seg != 0
    lat[::2, ::2] = fg
    lat[::2, 1::2] = fg[:, 1:] & (seg[:, 1:] == seg[:, :-1])
    lat[1::2, ::2] = fg[1:, :] & (seg[1:, :] == seg[:-1, :])
    lab, n = ndimage.label(lat)           # default structure: 4-connectivity; labels in raster order
    lab = lab[::2, ::2]
    if n and (h > 512 or w > 512):
        first = ndimage.minimum(_block_major_keys(h, w), lab, index=np.arange(1, n + 1))    # first block-major position per component
        rank = np.empty(n + 1, dtype=np.int64)
        rank[0] = 0
        rank[1 + np.argsort(first, kind="stable")] = np.arange(1, n + 1)
        lab = rank[lab]
    return lab.astype(seg.dtype)


def mask_data_to_segmentation(masks: List[Dict[str, Any]], shape: Optional[Tuple[int, int]] = None,
                              min_object_size: int = 0, max_object_size: Optional[int] = None, label_masks: bool = True,
                              with_background: bool = False, merge_exclusively: bool = True) -> np.ndarray:
    """Reference util.py:1773-1848."""
    masks = sorted(masks, key=(lambda x: x["area"]), reverse=True)
    if shape is None:
        shape = next(iter(masks))["segmentation"].shape
    segmentation = np.zeros(shape, dtype="uint32")

    def require_numpy(mask):
        return mask.cpu().numpy() if torch.is_tensor(mask) else mask

    seg_id = 1
    for mask_data in masks:
        area = mask_data["area"]
        if (area < min_object_size) or (max_object_size is not None and area > max_object_size):
            continue
        this_mask = require_numpy(mask_data["segmentation"])
        this_seg_id = mask_data.get("seg_id", seg_id)
        if "global_bbox" in mask_data:
            bb = mask_data["bbox"]
            bb = np.s_[bb[1]:bb[1] + bb[3], bb[0]:bb[0] + bb[2]]
            gbb = mask_data["global_bbox"]
            gbb = np.s_[gbb[1]:gbb[1] + gbb[3], gbb[0]:gbb[0] + gbb[2]]
            this_mask = np.logical_and(this_mask[bb], segmentation[gbb] == 0) if merge_exclusively else this_mask[bb]
            segmentation[gbb][this_mask] = this_seg_id
        else:
            if merge_exclusively:
                this_mask = np.logical_and(this_mask, segmentation == 0)
            segmentation[this_mask] = this_seg_id
        seg_id = this_seg_id + 1
    if label_masks:
        segmentation = _label_equal_value_components(segmentation)
    sizes = np.bincount(segmentation.ravel())
    seg_ids = np.nonzero(sizes)[0]
    sizes = sizes[seg_ids]
    filter_ids = seg_ids[sizes < min_object_size]
    if with_background:
        filter_ids = np.concatenate([filter_ids, [seg_ids[np.argmax(sizes)]]])
    lut = np.ones(int(segmentation.max()) + 1, dtype=bool)
    lut[filter_ids] = False
    lut[0] = False
    # zero the filtered ids, then relabel the survivors consecutively (order preserving, 0 stays 0)
    new_ids = np.zeros(lut.shape[0], dtype=segmentation.dtype)
    new_ids[lut] = np.arange(1, int(lut.sum()) + 1, dtype=segmentation.dtype)
    return new_ids[segmentation]


def _infer_tiled_shape(predictions) -> Tuple[int, int]:
    """Output shape spanned by tile-local records (reference util.py:1757-1766)."""
    height = width = 0
    for pred in predictions:
        (bx, by), (gx, gy) = pred["bbox"][:2], pred["global_bbox"][:2]
        mh, mw = pred["segmentation"].shape
        height, width = max(height, int(gy - by) + mh), max(width, int(gx - bx) + mw)
    return height, width


def _tiled_overlap_scores(masks: List[np.ndarray], boxes: np.ndarray, global_boxes: np.ndarray,
                          intersection_over_min: bool) -> Dict[Tuple[int, int], np.float32]:
    """Overlap score of every pair (i < j) of tile-local masks whose global boxes share area (reference
    ``_calculate_tiled_mask_overlap_matrix``, util.py:1769-1822): the two masks are compared on the intersection window
    of their global xywh boxes only, IoU or intersection over the smaller area in float32.  Sparse: pairs that are not
    returned score 0."""
    gx0, gy0 = global_boxes[:, 0], global_boxes[:, 1]
    gx1, gy1 = gx0 + global_boxes[:, 2], gy0 + global_boxes[:, 3]
    off_x, off_y = gx0 - boxes[:, 0], gy0 - boxes[:, 1]          # tile origin of every record in the image
    areas = np.array([m.sum() for m in masks], dtype=np.float32)
    scores = {}
    order = np.argsort(gx0, kind="stable")                        # sweep along x: candidates end once their x0 >= our x1
    sorted_x0 = gx0[order]
    for rank, i in enumerate(order):
        hi = np.searchsorted(sorted_x0, gx1[i], side="left")
        for j in order[rank + 1:hi]:
            wx0, wx1 = max(gx0[i], gx0[j]), min(gx1[i], gx1[j])
            wy0, wy1 = max(gy0[i], gy0[j]), min(gy1[i], gy1[j])
            if wx1 <= wx0 or wy1 <= wy0:
                continue
            a = masks[i][wy0 - off_y[i]:wy1 - off_y[i], wx0 - off_x[i]:wx1 - off_x[i]]
            b = masks[j][wy0 - off_y[j]:wy1 - off_y[j], wx0 - off_x[j]:wx1 - off_x[j]]
            inter = np.float32(np.count_nonzero(a & b))
            den = min(areas[i], areas[j]) if intersection_over_min else areas[i] + areas[j] - inter
            with np.errstate(divide="ignore", invalid="ignore"):
                scores[(min(i, j), max(i, j))] = np.float32(inter) / np.float32(den)
    return scores


def _tiled_candidate_pairs(global_boxes: np.ndarray) -> np.ndarray:
    """The pairs ``_tiled_overlap_scores`` scores, from the (int64) global xywh boxes alone: int32 [Np, 2] in the order of its sweep
    along x, only pairs whose window is not empty (a listed pair of two empty masks would turn 0/0 into a suppression)."""
    gx0, gy0 = global_boxes[:, 0], global_boxes[:, 1]
    gx1, gy1 = gx0 + global_boxes[:, 2], gy0 + global_boxes[:, 3]
    order = np.argsort(gx0, kind="stable")
    his = np.searchsorted(gx0[order], gx1[order], side="left")
    pairs = []
    for rank, i in enumerate(order):
        js = order[rank + 1:his[rank]]
        if js.size:
            hit = (np.minimum(gx1[i], gx1[js]) > np.maximum(gx0[i], gx0[js])) & (np.minimum(gy1[i], gy1[js]) > np.maximum(gy0[i], gy0[js]))
            js = js[hit]
            pairs.append(np.stack([np.full(js.shape, i), js], axis=1))
    return np.concatenate(pairs).astype(np.int32) if pairs else np.zeros((0, 2), np.int32)


class _TiledTable:
    """The record table of csrc/tilemerge.hip for tile-local records whose masks are dense device tensors: ``words`` (the bit masks
    of all records, packed on the device per run of equal tile shape), per record its first word, tile geometry and boxes, and
    ``areas`` (int64 [K] on the host: the popcount of every whole tile mask, counted on the device and downloaded once).  ``ok`` is
    False where a bbox leaves its tile, which the kernels' wrappers refuse."""

    def __init__(self, records):
        from ._propagate import MAX_OBJECTS, pack_bits
        masks = [r["segmentation"] for r in records]
        k = len(masks)
        self.boxes = np.array([r["bbox"] for r in records]).astype(np.int64).reshape(k, -1)[:, :4]          # .to(torch.long): truncation
        self.global_boxes = np.array([r["global_bbox"] for r in records]).astype(np.int64).reshape(k, -1)[:, :4]
        shapes = np.array([tuple(m.shape) for m in masks], dtype=np.int64).reshape(k, 2)
        wpc, tw = (shapes[:, 0] + 31) // 32, shapes[:, 1]
        self.word_offset = np.concatenate([[0], np.cumsum(wpc * tw)[:-1]]).astype(np.int64)
        words, areas = [], []
        s = 0
        while s < k:                                     # runs of equal tile shape, at most 64 MiB of dense masks per stack
            e, limit = s + 1, min(MAX_OBJECTS, max(1, (1 << 26) // max(1, int(shapes[s, 0] * shapes[s, 1]))))
            while e < k and e - s < limit and tuple(shapes[e]) == tuple(shapes[s]):
                e += 1
            stack = torch.stack([m if m.dtype == torch.bool else m != 0 for m in masks[s:e]])
            words.append(pack_bits(stack).reshape(-1))
            areas.append(stack.flatten(1).sum(dim=1, dtype=torch.int32))
            s = e
        self.words = torch.cat(words)
        self.areas = fetch_to_host(torch.cat(areas), tag="tile_areas").astype(np.int64)
        self.geom = np.concatenate([np.stack([wpc, tw], axis=1), self.boxes, self.global_boxes[:, :2]], axis=1)
        bx, by, bw, bh = (self.boxes[:, c] for c in range(4))
        self.ok = bool(np.all((bx >= 0) & (by >= 0) & (bw >= 0) & (bh >= 0) & (bx + bw <= tw) & (by + bh <= shapes[:, 0])
                              & (np.abs(self.global_boxes) < 2 ** 30).all(axis=1)))

    def inside(self, shape) -> bool:
        g = self.global_boxes
        return bool(np.all((g[:, 0] >= 0) & (g[:, 1] >= 0) & (g[:, 0] + self.boxes[:, 2] <= shape[1]) & (g[:, 1] + self.boxes[:, 3] <= shape[0])))

    def select(self, idx):
        idx = np.asarray(idx, dtype=np.int64)
        return self.word_offset[idx], np.ascontiguousarray(self.geom[idx].astype(np.int32))


def _merge_tiled_device(table: _TiledTable, paint_order, shape, min_object_size: int, seg_ids=None) -> Optional[np.ndarray]:
    """``mask_data_to_segmentation(records, shape, min_object_size)`` for the records ``paint_order`` of ``table`` (already in the
    stable area-descending paint order, records below ``min_object_size`` left out): msam_paint_tiled, then the device tail (component
    labelling, size filter, consecutive relabel) and ONE download.  ``seg_ids``: the value each of them paints (records of different
    tiles may share a ``seg_id``, and equal values that touch are one component); None: distinct values.  Returns None if the
    labelling reported an open edge (the caller repeats the merge on the host)."""
    from . import ops
    h, w = int(shape[0]), int(shape[1])
    m = len(paint_order)
    if m == 0:
        return np.zeros((h, w), dtype="uint32")
    off, geom = table.select(paint_order)
    painted = ops.paint_tiled(table.words, off, geom, np.arange(m, dtype=np.int32), h, w)
    if seg_ids is not None:                                                 # painted value M - r -> the record's seg_id
        lut = torch.tensor([0] + [int(v) for v in reversed(seg_ids)], dtype=torch.int32, device=painted.device)
        painted = lut[painted.to(torch.int64)]
    labels, flag = _painted_to_labels_device(painted, min_object_size)
    out = fetch_to_host(torch.cat([labels.reshape(-1), flag]), tag="labels")    # one download: the label image + the convergence flag
    if out[-1] != 0:
        return None
    return out[:-1].reshape(h, w).view(np.uint32)


def _apply_nms_tiled_device(predictions, min_size, shape, perform_box_nms, nms_thresh, max_size, intersection_over_min) -> Optional[np.ndarray]:
    """``_apply_nms_tiled`` for records whose masks are dense device tensors, without bringing a mask to the host: the masks are
    packed to bits where they are, the candidate pairs come from the boxes, ONE msam_tiled_mask_overlaps launch counts their window
    intersections, the scores and the greedy sweep (O(K + pairs) scalar work) stay on the host in the host path's float32
    arithmetic, and the survivors are merged by ``_merge_tiled_device``.  Returns None where the host path has to answer: a box
    that leaves its tile or ``shape`` (the host path raises or clips as before), or a labelling that did not converge."""
    from . import ops
    table = _TiledTable(predictions)
    if not (table.ok and table.inside(shape)):
        return None
    areas = table.areas
    sel = np.arange(len(predictions))
    if min_size > 0:
        sel = sel[areas[sel] > min_size]
    if max_size is not None:
        sel = sel[areas[sel] < max_size]
    if sel.size == 0:
        return np.zeros(shape, dtype="uint32")
    scores = np.array([np.float32(predictions[i]["predicted_iou"]) * np.float32(predictions[i]["stability_score"]) for i in sel],
                      dtype=np.float32)
    if perform_box_nms:
        dev = table.words.device
        xyxy = torch.tensor([predictions[i]["global_bbox"] for i in sel], dtype=torch.float32, device=dev)
        xyxy[:, 2] += xyxy[:, 0]
        xyxy[:, 3] += xyxy[:, 1]
        keep = ops.box_nms(xyxy, torch.as_tensor(scores, device=dev), nms_thresh).cpu().tolist()
    else:
        pairs = _tiled_candidate_pairs(table.global_boxes[sel])
        off, geom = table.select(sel)
        inter = fetch_to_host(ops.tiled_mask_overlaps(table.words, off, geom, pairs), tag="tile_inter").astype(np.float32)
        a = areas[sel].astype(np.float32)
        ai, aj = a[pairs[:, 0]], a[pairs[:, 1]]
        den = np.minimum(ai, aj) if intersection_over_min else ai + aj - inter
        with np.errstate(divide="ignore", invalid="ignore"):
            v = inter / den
        hit = pairs[~(v <= np.float32(nms_thresh))]                                     # nan (0/0) suppresses, as `<=` does
        partners = {}
        for i, j in hit.tolist():
            partners.setdefault(i, []).append(j)
            partners.setdefault(j, []).append(i)
        suppressed = np.zeros(sel.size, dtype=bool)
        keep = []
        for i in np.argsort(-scores.astype(np.float64), kind="stable").tolist():
            if suppressed[i]:
                continue
            keep.append(i)
            suppressed[partners.get(i, [])] = True
    kept = [int(sel[i]) for i in keep]
    paint_order = [i for i in sorted(kept, key=lambda i: areas[i], reverse=True) if areas[i] >= min_size]
    return _merge_tiled_device(table, paint_order, shape, min_size)


def _apply_nms_tiled(predictions, min_size, shape, perform_box_nms, nms_thresh, max_size, intersection_over_min) -> np.ndarray:
    """``apply_nms`` for tile-local records (reference util.py:1876-1957 with ``is_tiled``).  Records whose masks are dense
    device tensors stay there (``_apply_nms_tiled_device``: msam_tiled_mask_overlaps + msam_paint_tiled); numpy / CPU records take
    the reference's host computation (``_batched_tiled_mask_nms`` moves everything to the CPU) below."""
    from . import ops
    if perform_box_nms and intersection_over_min:
        raise ValueError("intersection_over_min needs mask NMS (perform_box_nms=False)")
    if shape is None:
        shape = _infer_tiled_shape(predictions)
    if all(torch.is_tensor(p["segmentation"]) and p["segmentation"].is_cuda and p["segmentation"].dim() == 2 for p in predictions):
        out = _apply_nms_tiled_device(predictions, min_size, shape, perform_box_nms, nms_thresh, max_size, intersection_over_min)
        if out is not None:
            return out

    def dense(p):
        m = p["segmentation"]
        return (m.cpu().numpy() if torch.is_tensor(m) else np.asarray(m)).astype(bool)
    preds = [dict(p, segmentation=dense(p)) for p in predictions]
    for p in preds:
        p["area"] = int(p["segmentation"].sum())
    if min_size > 0:
        preds = [p for p in preds if p["area"] > min_size]
    if max_size is not None:
        preds = [p for p in preds if p["area"] < max_size]
    if not preds:
        return np.zeros(shape, dtype="uint32")
    scores = np.array([np.float32(p["predicted_iou"]) * np.float32(p["stability_score"]) for p in preds], dtype=np.float32)
    if perform_box_nms:
        dev = _lib.require_gpu()
        xyxy = torch.tensor([p["global_bbox"] for p in preds], dtype=torch.float32, device=dev)
        xyxy[:, 2] += xyxy[:, 0]
        xyxy[:, 3] += xyxy[:, 1]
        keep = ops.box_nms(xyxy, torch.as_tensor(scores, device=dev), nms_thresh).cpu().tolist()
    else:
        boxes = np.array([p["bbox"] for p in preds]).astype(np.int64)                   # .to(torch.long): truncation
        global_boxes = np.array([p["global_bbox"] for p in preds]).astype(np.int64)
        overlap = _tiled_overlap_scores([p["segmentation"] for p in preds], boxes, global_boxes, intersection_over_min)
        suppressed = np.zeros(len(preds), dtype=bool)
        partners = {}
        for (i, j), v in overlap.items():
            if not (v <= np.float32(nms_thresh)):                                       # nan (0/0) suppresses, as `<=` does
                partners.setdefault(i, []).append(j)
                partners.setdefault(j, []).append(i)
        keep = []
        for i in np.argsort(-scores.astype(np.float64), kind="stable").tolist():
            if suppressed[i]:
                continue
            keep.append(i)
            suppressed[partners.get(i, [])] = True
    records = [{k: preds[i][k] for k in ("segmentation", "area", "bbox", "global_bbox")} for i in keep]
    return mask_data_to_segmentation(records, shape=shape, min_object_size=min_size)


@torch.no_grad()
def apply_nms(predictions: List[Dict[str, Any]], min_size: int, shape: Optional[Tuple[int, int]] = None,
              perform_box_nms: bool = False, nms_thresh: float = 0.9, max_size: Optional[int] = None,
              intersection_over_min: bool = False) -> np.ndarray:
    """Reference ``util.apply_nms`` (micro_sam/util.py:1851-1957) for full-image predictions (records with a dense
    ``segmentation``, ``bbox`` xywh, ``predicted_iou``, ``stability_score``): size filters, NMS on
    score = predicted_iou * stability_score - box NMS (``msam_box_nms``) or mask NMS on IoU / intersection-over-min
    (``msam_mask_nms``: popcount of AND over bit masks instead of the reference's ``masks_flat @ masks_flat.T``) - and merge
    of the survivors to a label image.  Tile-local predictions (records with a ``global_bbox``, as
    ``inference.batched_tiled_inference`` returns them) go to ``_apply_nms_tiled``: with dense device masks the cross-tile
    window overlaps and the merge run on the device (``msam_tiled_mask_overlaps``, ``msam_paint_tiled``) and no mask is copied
    to the host; numpy / CPU records take the reference's host computation."""
    from . import ops
    from ._vendored import pack_bits
    if len(predictions) == 0:
        return np.zeros(shape, dtype="uint32")
    if "global_bbox" in predictions[0]:
        return _apply_nms_tiled(predictions, min_size, shape, perform_box_nms, nms_thresh, max_size, intersection_over_min)
    if perform_box_nms and intersection_over_min:
        raise ValueError("intersection_over_min needs mask NMS (perform_box_nms=False)")

    def dense(p):
        m = p["segmentation"]
        return m.cpu().numpy() if torch.is_tensor(m) else np.asarray(m)
    preds = [dict(p, area=int(dense(p).sum())) for p in predictions]
    if shape is None:
        shape = dense(predictions[0]).shape
    if min_size > 0:
        preds = [p for p in preds if p["area"] > min_size]
    if max_size is not None:
        preds = [p for p in preds if p["area"] < max_size]
    if not preds:
        return np.zeros(shape, dtype="uint32")
    dev = _lib.require_gpu()
    scores = torch.tensor([float(np.float32(p["predicted_iou"]) * np.float32(p["stability_score"])) for p in preds],
                          dtype=torch.float32, device=dev)
    xyxy = torch.tensor([p["bbox"] for p in preds], dtype=torch.float32, device=dev)
    xyxy[:, 2] += xyxy[:, 0]
    xyxy[:, 3] += xyxy[:, 1]
    if perform_box_nms:
        keep = ops.box_nms(xyxy, scores, nms_thresh)
    else:
        areas = torch.tensor([p["area"] for p in preds], dtype=torch.int32, device=dev)
        bits = torch.cat([pack_bits(torch.as_tensor(np.stack([dense(p) for p in preds[s:s + 64]]).astype(bool), device=dev))
                          for s in range(0, len(preds), 64)])
        keep = ops.mask_nms(bits, xyxy, areas, scores, nms_thresh, shape[0], intersection_over_min)
    kept = [preds[int(i)] for i in keep.cpu().tolist()]
    records = [{k: p[k] for k in ("segmentation", "area", "bbox")} for p in kept]
    return mask_data_to_segmentation(records, shape=shape, min_object_size=min_size)


def _root_marks(roots: torch.Tensor) -> torch.Tensor:
    """``ops.label_components`` gives every pixel the KEY of its component's root (-1: background; keys = positions in the
    reference's block-major numbering order, csrc/common.h bm_key).  Returns bool [n]: True at the keys that are roots - no
    data-dependent shape, no host synchronisation."""
    marks = torch.zeros(roots.numel() + 1, dtype=torch.bool, device=roots.device)
    marks[roots + 1] = True
    return marks[1:]


def mask_data_to_segmentation_device(bits: torch.Tensor, areas: torch.Tensor, shape: Tuple[int, int],
                                     min_object_size: int = 0, with_background: bool = False) -> np.ndarray:
    """``mask_data_to_segmentation(..., label_masks=True, merge_exclusively=False)`` (reference util.py:1773-1848) computed
    on the device from bit masks [K, ceil(H/32), W] and their areas [K]; returns the uint32 label image on the host.

    Same semantics as the host function above: stable area-descending paint order, later masks overwrite, 4-connected
    components of equal value numbered as ``elf.parallel.label(block_shape=(512, 512))`` numbers them (block by block, raster
    order of the first pixel inside a block: csrc/common.h bm_key), drop components smaller than
    ``min_object_size`` and (``with_background``) the largest one counting label 0, relabel consecutively."""
    from . import ops
    h, w = int(shape[0]), int(shape[1])
    dev = bits.device
    k = int(bits.shape[0])
    if k == 0:
        return np.zeros((h, w), dtype="uint32")
    areas = areas.to(dev)
    # stable area-descending paint order; masks below min_object_size sink to the end and are cut off by k_dev (no compaction,
    # no host synchronisation before the single download of the result)
    sel = areas >= min_object_size if min_object_size > 0 else torch.ones_like(areas, dtype=torch.bool)
    key = torch.where(sel, areas.to(torch.int64), torch.full((k,), -1, dtype=torch.int64, device=dev))
    order = torch.sort(key, descending=True, stable=True).indices.to(torch.int32)
    k_dev = sel.sum().to(torch.int32).reshape(1)
    labels, flag = ops.labels_from_masks(bits, order, (h, w), k_dev=k_dev, min_object_size=min_object_size,
                                         with_background=with_background)
    out = fetch_to_host(torch.cat([labels.reshape(-1), flag]), tag="labels")    # one download: the label image + the convergence flag
    if out[-1] != 0:                                                       # the labelling reported an open edge: repeat it on the host's clock
        return _mask_data_to_segmentation_device_iterative(bits, areas, shape, min_object_size, with_background)
    return out[:-1].reshape(h, w).view(np.uint32)


def _mask_data_to_segmentation_device_iterative(bits: torch.Tensor, areas: torch.Tensor, shape: Tuple[int, int],
                                                min_object_size: int = 0, with_background: bool = False) -> np.ndarray:
    """The same result with the union passes repeated until none changes anything (a host synchronisation per pass) and the
    relabelling as torch operators: the fallback of ``mask_data_to_segmentation_device`` and its cross-check in the tests."""
    from . import ops
    h, w = int(shape[0]), int(shape[1])
    dev = bits.device
    order = torch.sort(areas.to(dev), descending=True, stable=True).indices
    if min_object_size > 0:
        order = order[areas.to(dev)[order] >= min_object_size]
    painted = ops.paint_label_image(bits, order, h, w)
    roots = ops.label_components(painted).to(torch.int64)
    fg = roots >= 0
    is_root = _root_marks(roots)
    comp_of_root = torch.cumsum(is_root.to(torch.int64), 0)                  # 1..C at the root keys (the reference's block-major order)
    cid = torch.where(fg, comp_of_root[roots.clamp(min=0)], torch.zeros_like(roots))
    n_comp = int(comp_of_root[-1].item())
    sizes = torch.bincount(cid, minlength=n_comp + 1)
    keep = torch.ones(n_comp + 1, dtype=torch.bool, device=dev)
    keep[0] = False
    keep &= sizes >= min_object_size
    if with_background:
        present = sizes > 0                                                  # np.unique only reports ids that occur
        masked = torch.where(present, sizes, torch.full_like(sizes, -1))
        keep[int(torch.argmax(masked).item())] = False                       # first maximum = smallest id on ties
    new_id = torch.cumsum(keep.to(torch.int64), 0) * keep
    return new_id[cid].reshape(h, w).to(torch.int32).cpu().numpy().astype("uint32")


@torch.no_grad()
def masks_to_segmentation_device(bits: torch.Tensor, areas: torch.Tensor, keep: torch.Tensor, shape: Tuple[int, int],
                                 min_object_size: int = 0, with_background: bool = False):
    """Sync-free variant of ``mask_data_to_segmentation_device`` over ALL candidate masks with a boolean ``keep`` vector
    (the survivors of the threshold filters and NMS): no compaction, no host round trip.

    Returns (labels int32 [H,W] on the device, converged flag tensor int32[1] - must read 0)."""
    from . import ops
    h, w = int(shape[0]), int(shape[1])
    dev = bits.device
    n = int(bits.shape[0])
    if n == 0:
        return torch.zeros((h, w), dtype=torch.int32, device=dev), torch.zeros((1,), dtype=torch.int32, device=dev)
    areas = areas.to(dev)
    sel = keep & (areas >= min_object_size) if min_object_size > 0 else keep
    # stable area-descending order of the selected masks; unselected ones sink to the end and are cut off by k_dev
    key = torch.where(sel, areas.to(torch.int64), torch.full((n,), -1, dtype=torch.int64, device=dev))
    order = torch.sort(key, descending=True, stable=True).indices.to(torch.int32).contiguous()
    k_dev = sel.sum().to(torch.int32).reshape(1)
    painted = ops.paint_label_image_dev(bits, order, k_dev, h, w)
    return _painted_to_labels_device(painted, min_object_size, with_background)


def _painted_to_labels_device(painted: torch.Tensor, min_object_size: int = 0, with_background: bool = False):
    """The tail of ``mask_data_to_segmentation`` from a painted int32 [H,W] image on the device: 4-connected components of equal
    value in the reference's numbering, drop the components smaller than ``min_object_size`` and (``with_background``) the largest
    one counting label 0, relabel consecutively.  Returns (labels int32 [H,W], converged flag int32[1] - must read 0); no host
    synchronisation."""
    from . import ops
    h, w = int(painted.shape[0]), int(painted.shape[1])
    dev = painted.device
    roots32, flag = ops.label_components_async(painted, passes=2)
    roots = roots32.to(torch.int64)
    fg = roots >= 0
    safe_roots = roots.clamp(min=0)
    # component sizes keyed by root pixel index (no compaction): sizes[r] for roots, 0 elsewhere
    sizes32, bg32 = ops.component_sizes(roots32)
    sizes = sizes32.to(torch.int64)
    idx = torch.arange(h * w, device=dev)
    is_root = _root_marks(roots)
    keep_root = is_root & (sizes >= min_object_size)
    if with_background:
        bg_size = bg32[0].to(torch.int64)
        best = torch.argmax(sizes)                          # first maximum = smallest root key = smallest component id
        # NB: ``sizes[best]`` with a 0-dim index tensor is an ``item()`` call = a host synchronisation (measured: the host
        # waited for the whole decode of the tile here); the value at the first maximum is the maximum
        drop_component = sizes.max() > bg_size              # label 0 wins ties (it is the smallest id)
        keep_root = keep_root & ~((idx == best) & drop_component)
    new_id = torch.cumsum(keep_root.to(torch.int64), 0) * keep_root      # consecutive ids in ascending order of the root keys
    labels = torch.where(fg, new_id[safe_roots], torch.zeros_like(roots))
    return labels.reshape(h, w).to(torch.int32), flag
