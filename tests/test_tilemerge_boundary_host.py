"""The boundary of ``ops.tiled_mask_overlaps`` / ``ops.paint_tiled`` (micro_sam_amd/_tilemerge.py), checked the way
tests/test_ops_boundary_host.py checks the wrappers defined in ops.py itself, with the same recorder and the same single-fault mutations
(tests/ops_boundary_table.py): valid arguments reach msam_tiled_mask_overlaps / msam_paint_tiled with the expected scalars, and every
single fault - a wrong type, rank, size, stride or device of ``words``, a host table the kernels could not trust - is refused before any
library call, with a message that names the argument.  Also here, without a GPU: the candidate pairs of the device path are the pairs
the host path scores."""
import re

import numpy as np
import pytest
import torch

import tiled_merge_cases as T
from ops_boundary_table import Entry, i32, mutations, recording, z

GEOM = np.array([[2, 50, 4, 6, 20, 40, 10, 12], [1, 30, 0, 0, 29, 31, 64, 0]], np.int32)      # tiles of 2 x 50 and 1 x 30 words
OFF = np.array([0, 100], np.int64)


def _geom(row, col, value):
    g = GEOM.copy()
    g[row, col] = value
    return g


_TABLE_FAULTS = [("bx < 0", {"geom": _geom(0, 2, -1)}, "geom"), ("bx + bw > tw", {"geom": _geom(1, 4, 31)}, "geom"),
                 ("by < 0", {"geom": _geom(1, 3, -1)}, "geom"), ("by + bh > 32 wpc", {"geom": _geom(1, 5, 33)}, "geom"),
                 ("wpc = 0", {"geom": _geom(0, 0, 0)}, "geom"), ("geom int64", {"geom": GEOM.astype(np.int64)}, "geom"),
                 ("geom [K, 7]", {"geom": np.ascontiguousarray(GEOM[:, :7])}, "geom"), ("geom a tensor", {"geom": torch.from_numpy(GEOM)}, "geom"),
                 ("offset past the words", {"word_offset": np.array([0, 101], np.int64)}, "word_offset"),
                 ("negative offset", {"word_offset": np.array([-1, 100], np.int64)}, "word_offset"),
                 ("offsets int32", {"word_offset": OFF.astype(np.int32)}, "word_offset"),
                 ("one offset", {"word_offset": OFF[:1].copy()}, "word_offset")]


def _check_overlaps(calls, kw):
    a = calls[0][1]
    assert a[0] == kw["words"].data_ptr() and (a[3], a[5]) == (2, 3) and a[7] is None


def _check_paint(calls, kw):
    a = calls[0][1]
    assert a[0] == kw["words"].data_ptr() and (a[4], a[5], a[6]) == (3, 60, 96) and a[8] is None


ENTRIES = [
    Entry("ops", "tiled_mask_overlaps",
          lambda: dict(words=z(130, dt=i32), word_offset=OFF.copy(), geom=GEOM.copy(), pairs=np.array([[0, 1], [1, 0], [1, 1]], np.int32)),
          ["msam_tiled_mask_overlaps"], check=_check_overlaps,
          scalars=_TABLE_FAULTS + [("a pair outside the table", {"pairs": np.array([[0, 2]], np.int32)}, "pairs"),
                                   ("a negative pair", {"pairs": np.array([[-1, 0]], np.int32)}, "pairs"),
                                   ("pairs int64", {"pairs": np.zeros((1, 2), np.int64)}, "pairs"),
                                   ("pairs [Np, 3]", {"pairs": np.zeros((1, 3), np.int32)}, "pairs")]),
    Entry("ops", "paint_tiled",
          lambda: dict(words=z(130, dt=i32), word_offset=OFF.copy(), geom=GEOM.copy(), order=np.array([1, 0, 1], np.int32), height=60, width=96),
          ["msam_paint_tiled"], check=_check_paint,
          scalars=_TABLE_FAULTS + [("order outside the table", {"order": np.array([2], np.int32)}, "order"),
                                   ("order int64", {"order": np.zeros(1, np.int64)}, "order"),
                                   ("a window below the image", {"height": 51}, "geom"), ("a window right of the image", {"width": 92}, "geom"),
                                   ("a negative gx", {"geom": _geom(0, 6, -1)}, "geom"), ("no rows", {"height": 0}, "height")]),
]
CASES = [(e, label) for e in ENTRIES for label, _, _ in mutations(e, e.build())]


@pytest.mark.parametrize("entry", ENTRIES, ids=[e.name for e in ENTRIES])
def test_valid_arguments_reach_the_kernel(entry):
    kw = entry.build()
    with recording() as rec:
        out = entry.fn()(**kw)
    assert rec.names() == entry.expect and out.dtype == torch.int32
    entry.check(rec.calls, kw)
    assert {"words:dtype", "words:strides", "words:rank", "words:device", "words:size0"} <= {label for label, _, _ in mutations(entry, kw)}


@pytest.mark.parametrize("entry,label", CASES, ids=[f"{e.name}-{label}" for e, label in CASES])
def test_single_fault_is_refused_before_any_call(entry, label):
    (name, kw), = [(n, k) for lab, n, k in mutations(entry, entry.build()) if lab == label]
    with recording() as rec:
        with pytest.raises((ValueError, TypeError)) as err:
            entry.fn()(**kw)
    assert not rec.calls, f"refused after {rec.names()}"
    assert re.search(rf"\b{name}\b", str(err.value)), f"the message does not name {name}: {err.value}"


def test_nothing_to_do_launches_nothing_or_only_the_memset():
    kw = ENTRIES[0].build()
    with recording() as rec:
        assert ENTRIES[0].fn()(**dict(kw, pairs=np.zeros((0, 2), np.int32))).shape == (0,)
    assert not rec.calls
    kw = ENTRIES[1].build()
    with recording() as rec:
        ENTRIES[1].fn()(**dict(kw, order=np.zeros(0, np.int32)))
    assert rec.names() == ["msam_paint_tiled"] and rec.calls[0][1][:5] == [None, None, None, None, 0]      # (zeroes the image)


@pytest.mark.parametrize("seed", T.SEEDS)
def test_candidate_pairs_are_the_pairs_the_host_path_scores(seed):
    from micro_sam_amd import util
    recs = T.tiled_records(seed)
    boxes = np.array([r["bbox"] for r in recs]).astype(np.int64)
    gboxes = np.array([r["global_bbox"] for r in recs]).astype(np.int64)
    scores = util._tiled_overlap_scores([r["segmentation"] for r in recs], boxes, gboxes, False)
    pairs = util._tiled_candidate_pairs(gboxes)
    assert pairs.dtype == np.int32 and len(pairs) == len(scores) > 100
    assert {(min(i, j), max(i, j)) for i, j in pairs.tolist()} == set(scores) == {tuple(p) for p in T.candidate_pairs(recs).tolist()}
    assert util._tiled_candidate_pairs(gboxes[:1]).shape == (0, 2)
