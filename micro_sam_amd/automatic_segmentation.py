"""The top-level entry point of automatic instance segmentation (reference ``micro_sam/automatic_segmentation.py``:
``get_predictor_and_segmenter`` :25-79, ``_add_suffix_to_output_path`` :82-85, ``automatic_instance_segmentation`` :171-327), with the
reference's signatures, defaults and messages.  It is a driver: the model and its state come from ``util.get_sam_model``, the generator
from ``get_instance_segmentation_generator``, a 2-d input runs ``initialize`` + ``generate``, a 3-d input runs
``multi_dimensional_segmentation.automatic_3d_segmentation`` (per-slice segmentation and, on a GPU, the merge across z on the device).

Not here: ``automatic_tracking`` / ``track_across_frames`` (Trackastra is absent) and the command-line ``main``."""
import os
from pathlib import Path
from typing import Optional, Tuple, Union

import numpy as np

from . import util
from .instance_segmentation import (DEFAULT_SEGMENTATION_MODE_WITH_DECODER, InstanceSegmentationWithDecoder, TiledAutomaticPromptGenerator,
                                    get_decoder, get_instance_segmentation_generator)
from .multi_dimensional_segmentation import automatic_3d_segmentation


def get_predictor_and_segmenter(model_type: str, checkpoint: Optional[Union[os.PathLike, str]] = None, device: str = None,
                                segmentation_mode: Optional[str] = None, is_tiled: bool = False, predictor=None, state=None,
                                **kwargs):
    """Reference :25-79: the predictor and the automatic instance segmentation class for it.  ``segmentation_mode`` is one of 'amg',
    'ais', 'apg'; by default (None or 'auto') 'ais' when the model's state holds a ``decoder_state``, else 'amg'.  A pre-loaded
    ``predictor`` needs its ``state``.  ``kwargs`` go to the generator class."""
    if predictor is None:
        device = util.get_device(device=device)
        predictor, state = util.get_sam_model(model_type=model_type, device=device, checkpoint_path=checkpoint, return_state=True)
    else:
        assert state is not None

    if segmentation_mode in (None, "auto"):
        segmentation_mode = DEFAULT_SEGMENTATION_MODE_WITH_DECODER if "decoder_state" in state else "amg"

    if segmentation_mode.lower() == "amg":
        decoder = None
    else:
        if "decoder_state" not in state:
            raise RuntimeError(f"You have passed 'segmentation_mode={segmentation_mode}', but your model does not contain a decoder.")
        decoder = get_decoder(image_encoder=predictor.model.image_encoder, decoder_state=state["decoder_state"], device=device)

    segmenter = get_instance_segmentation_generator(predictor=predictor, is_tiled=is_tiled, decoder=decoder,
                                                    segmentation_mode=segmentation_mode, **kwargs)
    return predictor, segmenter


def _add_suffix_to_output_path(output_path: Union[str, os.PathLike], suffix: str) -> str:
    fpath = Path(output_path).resolve()
    fext = fpath.suffix if fpath.suffix else ".tif"
    return str(fpath.with_name(f"{fpath.stem}{suffix}{fext}"))


def _write_segmentation(path: Union[str, os.PathLike], instances: np.ndarray) -> None:
    """One TIFF file that ``util.load_image_data`` reads back with equal values: through imageio when importable (the reference's
    ``imageio.imwrite(path, instances, compression="zlib")``), else through Pillow as 32-bit integer pages with deflate compression,
    one page per slice (a volume of one slice reads back as a single image).  Pillow's 32-bit pages are signed: ids above 2^31 - 1 are
    refused."""
    instances = np.asarray(instances)
    if instances.ndim not in (2, 3) or instances.dtype.kind not in "iub":
        raise ValueError(f"The segmentation must be a 2d or 3d integer array to be stored as tif, got {instances.dtype} {instances.shape}")
    try:
        import imageio.v3 as imageio
    except ImportError:
        imageio = None
    if imageio is not None:
        imageio.imwrite(path, instances, compression="zlib")
        return
    if instances.size and (int(instances.max()) > 2 ** 31 - 1 or int(instances.min()) < -2 ** 31):
        raise ValueError("The segmentation holds ids above 2^31 - 1, which the 32-bit integer pages of the tif writer cannot store.")
    from PIL import Image
    pages = [Image.fromarray(np.ascontiguousarray(p, dtype=np.int32)) for p in (instances if instances.ndim == 3 else instances[None])]
    if not pages:
        raise ValueError("The segmentation is empty.")
    pages[0].save(os.fspath(path), format="TIFF", compression="tiff_adobe_deflate", save_all=True, append_images=pages[1:])


def automatic_instance_segmentation(predictor, segmenter, input_path, output_path: Optional[Union[os.PathLike, str]] = None,
                                    embedding_path: Optional[Union[os.PathLike, str]] = None, mask_path=None,
                                    key: Optional[str] = None, mask_key: Optional[str] = None, ndim: Optional[int] = None,
                                    tile_shape: Optional[Tuple[int, int]] = None, halo: Optional[Tuple[int, int]] = None,
                                    verbose: bool = True, return_embeddings: bool = False, annotate: bool = False, batch_size: int = 1,
                                    **generate_kwargs):
    """Reference :171-327: automatic segmentation of an image or a volume.

    ``input_path`` is a file (read with ``util.load_image_data(input_path, key)``) or an array; ``mask_path`` likewise an optional
    foreground mask outside of which nothing is processed (2-d only).  ``ndim`` defaults to the data's (pass 2 for an RGB image).
    ``output_path``: where the result is stored, as one ``.tif`` (the suffix is forced); a result that is already there is not
    overwritten: the call prints where it is and returns None.  ``generate_kwargs`` go to the generator's ``generate`` (2-d) or to
    ``automatic_3d_segmentation`` (3-d: ``gap_closing``, ``min_z_extent``, ... and the generate arguments).  Returns the segmentation,
    with the image embeddings when ``return_embeddings``.

    Unlike the reference, ``annotate=True`` raises at entry, before anything is loaded or computed: there is no annotator (napari)
    here; the reference would open it after the segmentation."""
    if annotate:
        raise NotImplementedError("annotate=True needs the napari annotator, which micro_sam_amd does not have; "
                                  "run with annotate=False and open the stored segmentation in a viewer of your choice.")

    # Avoid overwriting already stored segmentations.
    if output_path is not None:
        output_path = Path(output_path).with_suffix(".tif")
        if os.path.exists(output_path):
            print(f"The segmentation results are already stored at '{os.path.abspath(output_path)}'.")
            return

    # A str or pathlike is read from file, anything else is taken as an array.
    image_data = util.load_image_data(input_path, key) if isinstance(input_path, (str, os.PathLike)) else input_path
    ndim = image_data.ndim if ndim is None else ndim

    if mask_path is None:
        mask = None
    else:
        mask = util.load_image_data(mask_path, mask_key) if isinstance(mask_path, (str, os.PathLike)) else mask_path

    if ndim == 2:
        if (image_data.ndim != 2) and (image_data.ndim != 3 and image_data.shape[-1] != 3):
            raise ValueError(f"The inputs does not match the shape expectation of 2d inputs: {image_data.shape}")

        image_embeddings = util.precompute_image_embeddings(predictor=predictor, input_=image_data, save_path=embedding_path, ndim=ndim,
                                                            tile_shape=tile_shape, halo=halo, verbose=verbose, batch_size=batch_size,
                                                            mask=mask)
        initialize_kwargs = dict(image=image_data, image_embeddings=image_embeddings, verbose=verbose)
        if mask is not None:
            initialize_kwargs["mask"] = mask

        # AIS with tiling uses the same tile shape for the watershed post-processing, and the batch size for the decoder.
        if isinstance(segmenter, InstanceSegmentationWithDecoder) and tile_shape is not None:
            if not isinstance(segmenter, TiledAutomaticPromptGenerator):
                generate_kwargs.update({"tile_shape": tile_shape, "halo": halo})
            initialize_kwargs["batch_size"] = batch_size

        segmenter.initialize(**initialize_kwargs)
        instances = segmenter.generate(**generate_kwargs)

    else:
        if (image_data.ndim != 3) and (image_data.ndim != 4 and image_data.shape[-1] != 3):
            raise ValueError(f"The inputs does not match the shape expectation of 3d inputs: {image_data.shape}")
        if mask is not None:
            raise NotImplementedError

        instances, image_embeddings = automatic_3d_segmentation(volume=image_data, predictor=predictor, segmentor=segmenter,
                                                                embedding_path=embedding_path, tile_shape=tile_shape, halo=halo,
                                                                verbose=verbose, return_embeddings=True, batch_size=batch_size,
                                                                **generate_kwargs)

    if output_path is not None:
        _write_segmentation(output_path, instances)
        if verbose:
            print(f"The automatic segmentation results are stored at '{os.path.abspath(output_path)}'.")

    if return_embeddings:
        return instances, image_embeddings
    return instances
