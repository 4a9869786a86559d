"""The point grids of the automatic mask generator on the device, with the part of the decode that depends on them alone.

``AutomaticMaskGenerator`` builds its point grids once and scales them by the crop size, so every tile, slice or frame of one size
decodes the same prompts.  Nothing in front of the decoder's layer-0 token->image attention reads the image
(``msam_decoder_prompt_prefix``, include/msam_hip.h): an entry of this cache keeps the uploaded point and label tensors of one grid
chunk and, where the kernel path decodes, the prefix block computed from them (``Sam.make_prompt_prefix``).
"""
from collections import OrderedDict
from typing import Any, Callable, Hashable, Optional, Tuple

import numpy as np

MAX_ENTRIES = 8         # one entry is 16.5 MB for 1024 single-point prompts


class PromptPrefixCache:
    """At most ``max_entries`` entries, dropped oldest first.

    An entry is ``(points, labels, prefix)`` as ``make(points_host)`` returned it; it is found again by ``key`` and by the host
    points themselves (compared element by element: two grids may share a key).  ``owner`` is the object the blocks were computed
    from - the decoder's prepared constants, which are rebuilt for new weights, another 16-bit layout or a PEFT merge -: the whole
    cache is dropped when another owner asks.  Whatever else decides what ``make`` returns (the device, whether a block is wanted)
    belongs in ``key``."""

    def __init__(self, max_entries: int = MAX_ENTRIES):
        self.max_entries = int(max_entries)
        self._owner = None
        self._entries: "OrderedDict[Hashable, Tuple[np.ndarray, Any]]" = OrderedDict()

    def __len__(self) -> int:
        return len(self._entries)

    def clear(self) -> None:
        self._entries.clear()
        self._owner = None

    def get(self, key: Hashable, points_host: np.ndarray, owner: Any, make: Callable[[np.ndarray], Any]):
        if owner is not self._owner:
            self._entries.clear()
            self._owner = owner
        hit: Optional[Tuple[np.ndarray, Any]] = self._entries.get(key)
        if hit is not None and np.array_equal(hit[0], points_host):
            return hit[1]
        value = make(points_host)
        self._entries.pop(key, None)
        while len(self._entries) >= self.max_entries:
            self._entries.popitem(last=False)
        self._entries[key] = (np.array(points_host, copy=True), value)
        return value
