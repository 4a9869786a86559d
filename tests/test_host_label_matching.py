"""msam_label_matching (csrc/matching.hip) in the host build of the library (tests/hip_host_shim.build_library), driven through the C ABI
as tests/test_host_library.py drives the other entry points, and compared integer for integer with tests/matching_ref.py (elf's dense
overlap matrix and linear_sum_assignment): the full contingency table read back from the workspace, the object counts, the areas, the
per-threshold edge counts and the edge list; scores derived from the edge list are compared as float64 BITS.
tests/test_gpu_evaluation.py runs the kernel cases on the device."""
import ctypes as C
import os

import numpy as np
import pytest

import matching_ref as R
from hip_host_shim import build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = C.c_void_p
HDR, ITEM, EDGE = 4, 20, 6                      # include/msam_hip.h MSAM_MATCH_HEADER / _ITEM / _EDGE
GUARD = 64                                      # guard words in front of and behind every buffer the library writes
G_WS, G_RES = 0x5A, -1234567


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    lib = build_library(str(tmp_path_factory.mktemp("host_lib")), ROOT)
    lib.msam_label_matching_workspace_bytes.restype = C.c_int64
    lib.msam_last_error.restype = C.c_char_p
    return lib


def run(lib, pred, gt, thresholds, cap=4096, max_edges=4096):
    """-> (return code, per-item [(n_pred, n_true, counts, edges, table)], overflow, guards intact)."""
    pred, gt = np.ascontiguousarray(pred, np.int32), np.ascontiguousarray(gt, np.int32)
    B, H, W = pred.shape
    T = len(thresholds)
    thr = (C.c_double * T)(*[float(t) for t in thresholds])
    need = int(lib.msam_label_matching_workspace_bytes(B, cap))
    assert need == 28 * B * cap
    ws = np.full(need + 2 * GUARD * 8, G_WS, np.uint8)
    n_res = HDR + B * ITEM + max_edges * EDGE
    res = np.full(n_res + 2 * GUARD, G_RES, np.int32)
    rc = lib.msam_label_matching(pred.ctypes.data_as(vp), gt.ctypes.data_as(vp), B, gt.shape[0], H, W, thr, T,
                                 vp(ws.ctypes.data + GUARD * 8), C.c_int64(need), cap, vp(res.ctypes.data + GUARD * 4), max_edges, None)
    intact = bool((ws[:GUARD * 8] == G_WS).all() and (ws[-GUARD * 8:] == G_WS).all() and (res[:GUARD] == G_RES).all()
                  and (res[-GUARD:] == G_RES).all())
    if rc != 0:
        return rc, None, None, intact
    r = res[GUARD:GUARD + n_res]
    slots = B * cap
    body = ws[GUARD * 8:GUARD * 8 + need]
    keys = body[:slots * 8].view(np.uint64).reshape(B, cap)
    counts = body[slots * 16:slots * 20].view(np.int32).reshape(B, cap)
    n_edges = int(r[0])
    overflow = bool(r[1]) or n_edges > max_edges or any(r[HDR + b * ITEM + 3] for b in range(B))
    all_edges = r[HDR + B * ITEM:].reshape(max_edges, EDGE)[:min(n_edges, max_edges)].astype(np.int64)
    items = []
    for b in range(B):
        it = r[HDR + b * ITEM:HDR + (b + 1) * ITEM]
        e = all_edges[all_edges[:, 0] == b][:, 1:]
        e = e[np.lexsort((e[:, 1], e[:, 0]))]
        used = keys[b] != np.uint64(0xFFFFFFFFFFFFFFFF)
        table = {(int(k >> np.uint64(32)), int(k & np.uint64(0xFFFFFFFF))): int(c) for k, c in zip(keys[b][used], counts[b][used])}
        items.append((int(it[0]), int(it[1]), it[4:4 + T].astype(np.int64), e, table))
    return rc, items, overflow, intact


def check(lib, pred, gt, thresholds=R.DEFAULT_THRESHOLDS, **kw):
    rc, items, overflow, intact = run(lib, pred, gt, thresholds, **kw)
    assert rc == 0, lib.msam_last_error().decode()
    assert intact and not overflow
    want = R.label_matching(pred, gt, thresholds)
    gt = np.asarray(gt)
    for b, ((n_pred, n_true, counts, edges, table), (w_pred, w_true, w_counts, w_edges)) in enumerate(zip(items, want)):
        assert table == R.pair_table(pred[b], gt[b if gt.shape[0] > 1 else 0]), b          # (a) background pairs included
        assert (n_pred, n_true) == (w_pred, w_true), b
        assert np.array_equal(counts, w_counts), (b, counts, w_counts)
        assert np.array_equal(edges, w_edges), b
        # the scores the host derives from the edge list are the restatement's, bit for bit
        s = R.scores(pred[b], gt[b if gt.shape[0] > 1 else 0])
        p_ids = np.setdiff1d(np.unique(pred[b]), [0])
        g_ids = np.setdiff1d(np.unique(gt[b if gt.shape[0] > 1 else 0]), [0])
        got = edges[:, 2] / np.maximum(edges[:, 3] + edges[:, 4] - edges[:, 2], 1e-7)
        ref = s[np.searchsorted(p_ids, edges[:, 0]), np.searchsorted(g_ids, edges[:, 1])]
        assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), b
    return items


@pytest.mark.parametrize("G", [1, 3])
def test_shifted_ellipses(lib, G):
    """96 x 128 (three workgroup spans) with about 20 ellipses against shifted copies, B = 3, one or three ground-truth images."""
    gt = np.stack([R.ellipses(96, 128, 20, seed=g) for g in range(G)])
    pred = np.stack([R.ellipses(96, 128, 20, seed=b if G == 3 else 0, shift=(1 + b, 2 - b)) for b in range(3)])
    items = check(lib, pred, gt)
    assert all(it[0] >= 10 and it[2][0] >= 5 for it in items)                 # (the case has objects and matches)


def test_odd_size(lib):
    """37 x 53 = 1961 pixels: no multiple of 4 (scalar loads), of a thread's 16 pixels or of a workgroup's 4096."""
    check(lib, R.ellipses(37, 53, 9, seed=3, shift=(1, 1))[None], R.ellipses(37, 53, 9, seed=3)[None])
    check(lib, R.ellipses(37, 52, 9, seed=4, shift=(1, 1))[None], R.ellipses(37, 52, 9, seed=4)[None])       # wide loads and a ragged tail


@pytest.mark.parametrize("name", ["one_prediction", "mirrored", "chain"])
def test_exact_ties(lib, name):
    pred, gt, n_edges, tp = R.tie_cases()[name]
    (n_pred, n_true, counts, edges, _), = check(lib, pred[None], gt[None], [0.5])
    assert counts[0] == n_edges == len(edges) and R.true_positives(R.scores(pred, gt), 0.5) == tp
    assert tp < min(n_pred, n_true) or name != "chain"


def test_extreme_ids(lib):
    pred = R.ellipses(40, 48, 3, seed=5, shift=(1, 0))
    gt = R.ellipses(40, 48, 3, seed=5)
    ids = np.array([0, 7, 1_000_003, 2 ** 31 - 1], np.int32)
    items = check(lib, ids[pred][None], ids[gt][None])
    assert items[0][0] == 3 and items[0][2][0] >= 1
    check(lib, ids[pred][None], ids[[0, 3, 1, 2]][gt][None])     # the largest id on the other side of the key


def test_crowded_lds_table(lib):
    """64 x 64, every pixel of both images its own id: 4096 distinct pairs in one workgroup's span, four times its LDS table."""
    pred = np.arange(1, 4097, dtype=np.int32).reshape(1, 64, 64)
    gt = pred[:, ::-1].copy() + 5000
    items = check(lib, pred, gt, cap=16384, max_edges=8192)
    assert items[0][0] == items[0][1] == 4096 and len(items[0][4]) == 4096 and items[0][2][-1] == 4096
    gt[0, 32:] = 0                                               # half of the predictions lose their partner
    items = check(lib, pred, gt, [0.5, 1.0], cap=16384, max_edges=8192)
    assert list(items[0][2]) == [2048, 2048] and items[0][1] == 2048


def test_objects_across_workgroups(lib):
    """80 x 128 = 2.5 workgroup spans of 32 rows: bands and one object over the whole height cross every boundary."""
    pred = np.zeros((80, 128), np.int32)
    gt = np.zeros((80, 128), np.int32)
    pred[5:75, 10:40] = 1
    gt[8:78, 12:44] = 9
    pred[20:50, 60:120] = 2
    gt[25:60, 50:110] = 4
    pred[60:, 60:] = 3
    items = check(lib, pred[None], gt[None], [0.3, 0.5, 0.75])
    assert items[0][0] == 3 and items[0][1] == 2


def test_empty_inputs(lib):
    lab = R.ellipses(32, 40, 4, seed=6)
    zero = np.zeros_like(lab)
    for pred, gt in ((zero, lab), (lab, zero), (zero, zero)):
        (n_pred, n_true, counts, edges, table), = check(lib, pred[None], gt[None])
        assert counts.sum() == 0 and len(edges) == 0 and sum(table.values()) == lab.size


def test_threshold_lists(lib):
    pred, gt = R.ellipses(48, 64, 12, seed=7, shift=(2, 1))[None], R.ellipses(48, 64, 12, seed=7)[None]
    a = check(lib, pred, gt, [0.3, 0.5, 0.9])
    b = check(lib, pred, gt, np.linspace(0.2, 0.95, 16))
    assert len(b[0][2]) == 16 and a[0][2][0] >= a[0][2][1] >= a[0][2][2]
    check(lib, pred, gt, [0.9, 0.3, 0.5])                        # unordered: the edge list follows the smallest


def test_too_small_a_capacity(lib):
    """More distinct pairs than slots, then more edges than the list holds: flagged, nothing written outside the buffers (guard words
    on both sides of workspace and result), and the repeat with larger buffers is right."""
    pred = np.arange(1, 4097, dtype=np.int32).reshape(1, 64, 64)
    rc, _, overflow, intact = run(lib, pred, pred, [0.5], cap=1024, max_edges=8192)
    assert rc == 0 and overflow and intact
    rc, _, overflow, intact = run(lib, pred, pred, [0.5], cap=16384, max_edges=100)
    assert rc == 0 and overflow and intact
    check(lib, pred, pred, [0.5], cap=16384, max_edges=4096)


def test_bad_arguments(lib):
    pred = np.zeros((2, 8, 8), np.int32)
    thr = (C.c_double * 17)(*([0.5] * 17))
    cap = 1024
    need = int(lib.msam_label_matching_workspace_bytes(2, cap))
    ws, res = np.zeros(need, np.uint8), np.zeros(HDR + 2 * ITEM + 16 * EDGE, np.int32)
    p, w, r = pred.ctypes.data_as(vp), ws.ctypes.data_as(vp), res.ctypes.data_as(vp)
    good = dict(pred=p, gt=p, B=2, G=2, H=8, W=8, thr=thr, T=2, ws=w, ws_bytes=need, cap=cap, res=r, max_edges=16)

    def call(**kw):
        a = dict(good, **kw)
        before = res.copy()
        rc = lib.msam_label_matching(a["pred"], a["gt"], a["B"], a["G"], a["H"], a["W"], a["thr"], a["T"], a["ws"], C.c_int64(a["ws_bytes"]),
                                     a["cap"], a["res"], a["max_edges"], None)
        return rc, lib.msam_last_error().decode(), np.array_equal(before, res)
    assert call()[0] == 0
    res[:] = 77
    bad = [dict(pred=None), dict(gt=None), dict(thr=None), dict(ws=None), dict(res=None), dict(B=0), dict(B=-1), dict(G=3), dict(G=0),
           dict(T=0), dict(T=17), dict(H=0), dict(W=-2), dict(H=1 << 16, W=1 << 15), dict(cap=1000), dict(cap=512, ws_bytes=1 << 30),
           dict(ws_bytes=need - 1), dict(max_edges=0)]
    for kw in bad:
        rc, msg, untouched = call(**kw)
        assert rc != 0 and "msam_label_matching" in msg and untouched, kw
    assert lib.msam_label_matching_workspace_bytes(0, cap) == 0 and lib.msam_label_matching_workspace_bytes(2, 1000) == 0
