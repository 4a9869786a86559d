"""Test helper of tests/test_ops_boundary_host.py and tests/test_gpu_ops_boundary.py: the recorder that stands in for the loaded
library, and the table of the public wrappers of micro_sam_amd.ops / micro_sam_amd.strict that hand a ``data_ptr()`` to it - valid
arguments per wrapper, the single-fault mutations derived from them, and the functions that hand over nothing (``EXEMPT``).
TEST INFRASTRUCTURE; what the table means is described in tests/test_ops_boundary_host.py."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

F32, BF16, FP8, F16 = 1, 2, 3, 4
f32, bf16, f16, i32, i64, u8 = torch.float32, torch.bfloat16, torch.float16, torch.int32, torch.int64, torch.uint8


# ------------------------------------------------------------------------------------------------------------- recorder

class Recorder:
    """Stands in for the loaded library: ``calls`` = [(name, args)], struct arguments as {field: value}."""
    # outputs a wrapper reads back on the host before it goes on: zeroed through the (host) address it was given
    ZERO = {"msam_rle_run_counts": lambda a: (a[4], 4 * a[1]), "msam_slice_overlaps": lambda a: (a[9], 8)}

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("msam_"):
            raise AttributeError(name)
        if name.endswith("_bytes"):
            return lambda *a: 64
        if name == "msam_decoder_dtype":
            return lambda: F16
        if name == "msam_last_error":
            return lambda: b""

        def call(*args):
            plain = []
            for a in args:
                obj = getattr(a, "_obj", None)                       # ctypes.byref(struct)
                if isinstance(obj, ctypes.Structure):
                    a = {f[0]: getattr(obj, f[0]) for f in obj._fields_}
                plain.append(a)
            self.calls.append((name, plain))
            if name in self.ZERO:
                addr, n = self.ZERO[name](plain)
                if addr and torch.device(self.device).type == "cpu":
                    ctypes.memset(addr, 0, n)
            return 0
        return call

    device = "cpu"

    def names(self):
        return [c[0] for c in self.calls]


@contextlib.contextmanager
def recording(real_gpu: bool = False):
    """Patch micro_sam_amd._lib so that nothing can be launched; ``real_gpu`` keeps the true ``require_gpu`` / stream accessors
    (the device file: tensors live on the GPU, the library still is the recorder)."""
    from micro_sam_amd import _lib
    saved = (_lib._lib, _lib.require_gpu, _lib.stream_ptr, _lib.ptr, torch.cuda.current_stream)
    rec = Recorder()
    _lib._lib = rec
    if real_gpu:
        rec.device = "cuda"
    else:
        class _Stream:
            cuda_stream = 0
        _lib.require_gpu = lambda device=None: torch.device("cpu") if device is None else torch.device(device)
        _lib.stream_ptr = lambda: None
        _lib.ptr = lambda t: None if t is None else t.data_ptr()
        torch.cuda.current_stream = lambda *a, **k: _Stream()
    try:
        yield rec
    finally:
        _lib._lib, _lib.require_gpu, _lib.stream_ptr, _lib.ptr, torch.cuda.current_stream = saved


# ------------------------------------------------------------------------------------------------------------- the table

def z(*shape, dt=f32):
    return torch.zeros(shape, dtype=dt)


def blob(n=64):
    return torch.zeros(n, dtype=u8)


class Entry:
    def __init__(self, module, name, build, expect, free=(), skip=None, scalars=(), check=None, blame=None):
        self.module, self.name, self.build, self.expect = module, name, build, expect
        self.free = set(free)               # "arg:dim": the wrapper takes any size there (it defines M, P, ...)
        self.skip = skip or {}              # "arg:kind" or "arg:*" -> reason the mutation is no fault
        self.scalars = scalars              # [(label, {kwarg: value, ...}, name the message must hold)]
        self.check = check                  # check(calls, kw): asserts on the recorded scalar arguments
        self.blame = blame or {}            # mutation label -> the argument the refusal names instead (a dimension two tensors share)

    @property
    def id(self):
        return f"{self.module}.{self.name}"

    def fn(self):
        import importlib
        return getattr(importlib.import_module("micro_sam_amd." + self.module), self.name)


def tensor_paths(kw):
    """[(display name, path)] of every tensor among the arguments (one level of tuples: strict.i2t_block's (weight, bias) pairs)."""
    out = []
    for k, v in kw.items():
        if isinstance(v, torch.Tensor):
            out.append((k, (k,)))
        elif isinstance(v, (tuple, list)):
            out.extend((f"{k}[{i}]", (k, i)) for i, e in enumerate(v) if isinstance(e, torch.Tensor))
    return out


def get_path(kw, path):
    v = kw[path[0]]
    return v if len(path) == 1 else v[path[1]]


def set_path(kw, path, t):
    kw = dict(kw)
    if len(path) == 1:
        kw[path[0]] = t
    else:
        seq = list(kw[path[0]])
        seq[path[1]] = t
        kw[path[0]] = tuple(seq)
    return kw


def non_contiguous(t):
    if t.dim() == 0 or t.numel() <= 1:
        return None
    if t.shape[-1] > 1:
        v = torch.zeros(tuple(t.shape[:-1]) + (2 * t.shape[-1],), dtype=t.dtype, device=t.device)[..., ::2]
    else:
        d = max(i for i in range(t.dim()) if t.shape[i] > 1)
        shape = list(t.shape)
        shape[d] *= 2
        v = torch.zeros(shape, dtype=t.dtype, device=t.device).narrow(d, 0, t.shape[d]) if d else None
        if v is None or v.is_contiguous():
            v = torch.zeros(shape, dtype=t.dtype, device=t.device)[::2]
    assert tuple(v.shape) == tuple(t.shape) and not v.is_contiguous()
    return v


def mutations(entry, kw):
    """[(label, display name, mutated kwargs)]: the single faults of one entry."""
    out = []
    for name, path in tensor_paths(kw):
        t = get_path(kw, path)
        if f"{name}:*" in entry.skip:
            continue
        kinds = [("dtype", lambda t=t: t.to(torch.float32 if t.dtype == torch.float64 else torch.float64)),
                 ("strides", lambda t=t: non_contiguous(t)),
                 ("rank", lambda t=t: t.unsqueeze(0)),
                 ("device", lambda t=t: t.to("meta"))]
        for d in range(t.dim()):
            if f"{name}:{d}" not in entry.free:
                kinds.append((f"size{d}", lambda t=t, d=d: t.narrow(d, 0, t.shape[d] - 1).contiguous()))
        for kind, make in kinds:
            if f"{name}:{kind}" in entry.skip:
                continue
            m = make()
            if m is not None:
                out.append((f"{name}:{kind}", entry.blame.get(f"{name}:{kind}", name), set_path(kw, path, m)))
    for label, change, name in entry.scalars:
        m = dict(kw)
        for k, v in change.items():
            m[k] = v(kw) if callable(v) else v
        out.append((label, name, m))
    return out


def _p(calls, i=0):
    return calls[i][1]


def _gemm_check(calls, kw):
    p = _p(calls)[0]
    M, K = kw["a"].shape
    N = kw["w"].shape[0]
    assert (p["M"], p["N"], p["K"], p["lda"], p["ldw"], p["ldc"]) == (M, N, K, K, K, N)
    assert p["a_dtype"] == (F16 if kw["a"].dtype == f16 else 0) and p["out_dtype"] == {f32: F32, bf16: BF16, f16: F16}[kw["out_dtype"]]
    assert (p["resid_dtype"], p["resid_rows"], p["ldr"]) == (BF16, 8, N) and (p["table_rows"], p["table_cols"], p["table_ld"]) == (8, 64, 128)
    assert p["ln_mode"] == 1 and p["out_mode"] == 0


def _gemm_fp8_check(calls, kw):
    p = _p(calls)[0]
    assert (p["M"], p["N"], p["K"], p["lda"], p["ldw"], p["ldc"], p["ldr"]) == (16, 256, 128, 128, 128, 256, 256)
    assert p["a_dtype"] == FP8 and p["out_dtype"] == F16 and p["resid_dtype"] == F32 and p["resid_rows"] == 0


def _qkv_check(calls, kw):
    p = _p(calls)[0]
    assert (p["M"], p["N"], p["K"], p["lda"], p["ldw"]) == (32, 384, 64, 64, 64)
    assert (p["out_mode"], p["heads"], p["head_dim"], p["tokens"], p["a_dtype"]) == (1, 2, 64, 16, 0)


def _kv_check(calls, kw):
    p = _p(calls)[0]
    assert (p["M"], p["N"], p["K"], p["out_mode"], p["tokens"], p["table_rows"], p["table_cols"], p["table_ld"]) == (256, 256, 64, 2, 128, 128, 128, 128)
    assert p["a_dtype"] == 0


def _ln_check(calls, kw):
    a = _p(calls)
    assert (a[4], a[5], a[7], a[8], a[9]) == (6, 64, F16, 1, 0)


def _ct_check(calls, kw):
    a = _p(calls)
    assert (a[1], a[2], a[3], a[4]) == (F32, 5, 8, 8)


def _attn_check(calls, kw):
    a = _p(calls)
    n = 6 if len(a) == 13 else 5
    assert (a[n], a[n + 1], a[n + 2], a[n + 4]) == (1, 2, 64, BF16) and abs(a[n + 3] - 0.125) < 1e-7


def _sgemm_check(calls, kw):
    p = _p(calls)[0]
    assert (p["M"], p["N"], p["K"], p["lda"], p["ldw"], p["ldc"], p["ldr"], p["lda2"]) == (6, 16, 8, 8, 8, 16, 16, 8)
    assert (p["a2_rows"], p["res_rows"], p["split16"]) == (3, 0, 0)


def _wsgemm_kw():
    return dict(a=z(8, 64, dt=f16), w=z(128, 64, dt=f16), bias=z(128), table=z(4, 128), table_cols=64, resid=z(4, 128, dt=f16),
                resid_rows=4, ln_mode=2, ln_w=z(64), ln_b=z(64), out=z(8, 128, dt=f16))


def _fold_kw():
    return dict(ktok=z(2, 5, 128, dt=f16), vtok=z(2, 5, 128, dt=f16), wq=z(128, 256, dt=f16), wo=z(256, 128, dt=f16), bo=z(256))


def _chain2_kw():
    return dict(src=z(4096, 256, dt=f16), wv=z(128, 256, dt=f16), bv=z(128), wk=z(128, 256, dt=f16), ln0_w=z(256), ln0_b=z(256),
                wo0=z(256, 128, dt=f16), bo0=z(256))


def _objfeat_kw():
    desc = np.zeros((1, 12), np.int64)
    desc[0] = (0, 4, 4, 4, 0, 64, 4, 4, 0, 0, 0, 64)
    return dict(labels=z(16, dt=i64), ids=torch.ones(2, dtype=i64), emb=z(64 * 64 * 256), desc=desc, itab=np.zeros(24, np.int32),
                ftab=np.zeros(8, np.float32), sums=z(2, 256, dt=torch.float64), area_total=z(2, dt=i64), out=z(2, 257))


CONVERTED = "the wrapper converts this argument (type, layout and, where stated, device) before the hand-over"
ANY_SHAPE = "any shape: the kernel walks numel() elements"
BLOB = "a byte blob: only its length is checked, and it is flat by construction"

TABLE = [
    Entry("ops", "gemm", lambda: dict(a=z(8, 64, dt=f16), w=z(256, 64, dt=f16), bias=z(256), out_dtype=bf16, resid=z(8, 256, dt=bf16),
                                      resid_rows=8, table=z(8, 128), table_cols=64, out=z(8, 256, dt=bf16), ln_mode=1, ln_w=z(256), ln_b=z(256)),
          ["msam_gemm_bf16"], free={"a:0", "w:0", "table:0", "table:1"}, check=_gemm_check,
          blame={"a:size1": "w"},
          scalars=[("resid_rows > resid.shape[0]", {"resid_rows": 9}, "resid"), ("M > resid.shape[0]", {"resid_rows": 0, "resid": z(7, 256, dt=bf16)}, "resid"),
                   ("table_cols > table.shape[1]", {"table_cols": 192}, "table"),
                   ("out int32", {"out": z(8, 256, dt=i32)}, "out"), ("w fp32 with bf16 a", {"a": z(8, 64, dt=bf16), "w": z(256, 64)}, "w"),
                   ("ln_w missing", {"ln_w": None}, "ln_w")]),
    Entry("ops", "quant_rows_fp8", lambda: dict(x=z(4, 128, dt=bf16)), ["msam_quant_rows_fp8"], free={"x:0", "x:1"}),
    Entry("ops", "layernorm_fp8", lambda: dict(x=z(4, 768), weight=z(768), bias=z(768)), ["msam_layernorm_fp8"], free={"x:0", "x:1"}),
    Entry("ops", "gemm_fp8", lambda: dict(a8=z(16, 128, dt=torch.float8_e4m3fn), a_scale=z(16), w8=z(256, 128, dt=torch.float8_e4m3fn), w_scale=z(256),
                                          bias=z(256), resid=z(16, 256), out=z(16, 256, dt=f16)),
          ["msam_gemm_bf16"], free={"a8:0", "w8:0"}, check=_gemm_fp8_check, blame={"a8:size1": "w8"},
          scalars=[("out_dtype int8", {"out": None, "out_dtype": torch.int8}, "out")]),
    Entry("ops", "gemm_qkv", lambda: dict(a=z(32, 64, dt=bf16), w=z(384, 64, dt=bf16), bias=z(384), B=2, heads=2), ["msam_gemm_bf16"],
          free={"a:0", "w:0"}, check=_qkv_check, blame={"a:size1": "w"},
          scalars=[("fp16 operands", {"a": z(32, 64, dt=f16), "w": z(384, 64, dt=f16)}, "a"), ("fp32 operands", {"a": z(32, 64), "w": z(384, 64)}, "a"),
                   ("B does not divide M", {"B": 3}, "B"), ("3 * heads does not divide N", {"heads": 5}, "heads")]),
    Entry("ops", "gemm_kv", lambda: dict(a=z(256, 64, dt=bf16), w=z(256, 64, dt=bf16), bias=z(256), table=z(128, 128), tokens=128), ["msam_gemm_bf16"],
          free={"a:0", "table:0"}, check=_kv_check, blame={"a:size1": "w"},
          scalars=[("fp16 operands", {"a": z(256, 64, dt=f16), "w": z(256, 64, dt=f16)}, "a"), ("tokens does not divide M", {"tokens": 96}, "tokens")]),
    Entry("ops", "layernorm", lambda: dict(x=z(6, 64), weight=z(64), bias=z(64), eps=1e-6, out_dtype=f16, gelu=True), ["msam_layernorm"],
          free={"x:0", "x:1"}, check=_ln_check,
          scalars=[("out_dtype fp64", {"out_dtype": torch.float64}, "out_dtype"), ("nchw_hw does not divide rows", {"nchw_hw": 4}, "nchw_hw")]),
    Entry("ops", "cast_transpose", lambda: dict(x=z(5, 8), want_sum=True), ["msam_cast_transpose"], free={"x:0", "x:1"}, check=_ct_check),
    Entry("ops", "to_image", lambda: dict(x=z(4, 6, 3)), ["msam_to_image"],
          skip={"x:dtype": CONVERTED, "x:strides": CONVERTED, "x:rank": "a 2-d input gains a channel axis; the 4-d refusal (the reference's message) is below"},
          free={"x:0", "x:1", "x:2"}, scalars=[("4-d input", {"x": z(1, 4, 6, 3)}, "dimensionality")]),
    Entry("ops", "resize_bilinear_u8", lambda: dict(images=z(1, 4, 6, 3, dt=u8), newh=2, neww=3), ["msam_resample_u8", "msam_resample_u8"],
          free={"images:0", "images:1", "images:2", "images:3"}, skip={"images:strides": CONVERTED}),
    Entry("ops", "patchify", lambda: dict(img=z(1, 3, 1024, 1024)), ["msam_patchify"], free={"img:0"},
          check=lambda calls, kw: _p(calls)[1] == 1 or pytest.fail("B"),
          scalars=[("512 x 512 image", {"img": z(1, 3, 512, 512)}, "img"), ("channels-last image", {"img": z(1, 1024, 1024, 3).permute(0, 3, 1, 2)}, "img")]),
    Entry("ops", "patchify_u8", lambda: dict(img=z(1, 20, 30, 3, dt=u8)), ["msam_patchify_u8"], free={"img:0", "img:1", "img:2"},
          check=lambda calls, kw: tuple(_p(calls)[1:4]) == (1, 20, 30) or pytest.fail("B, h, w"),
          scalars=[("image taller than 1024", {"img": z(1, 1025, 8, 3, dt=u8)}, "img")]),
    Entry("ops", "im2col3x3", lambda: dict(x=z(1, 64, 64, 8, dt=bf16)), ["msam_im2col3x3"], free={"x:0", "x:3"},
          check=lambda calls, kw: tuple(_p(calls)[1:3]) == (1, 8) or pytest.fail("B, C"),
          scalars=[("grid 32 x 32", {"x": z(1, 32, 32, 8, dt=bf16)}, "x"), ("C % 8", {"x": z(1, 64, 64, 12, dt=bf16)}, "x")]),
    Entry("ops", "window_attention", lambda: dict(q=z(1, 2, 4096, 64, dt=bf16), k=z(1, 2, 4096, 64, dt=bf16), v=z(1, 2, 4096, 64, dt=bf16),
                                                  rel_h=z(27, 64, dt=bf16), rel_w=z(27, 64, dt=bf16), qkv_bias=z(384)), ["msam_window_attention16"],
          free={"q:0", "q:1"}, check=_attn_check,
          scalars=[("permuted q", {"q": z(1, 4096, 2, 64, dt=bf16).permute(0, 2, 1, 3)}, "q"),
                   ("hd 80", {n: z(1, 2, 4096, 80, dt=bf16) for n in "qkv"}, "q"), ("fp16 k with bf16 q", {"k": z(1, 2, 4096, 64, dt=f16)}, "k")]),
    Entry("ops", "global_attention", lambda: dict(q=z(1, 2, 4096, 64, dt=bf16), k=z(1, 2, 4096, 64, dt=bf16), v=z(1, 2, 4096, 64, dt=bf16),
                                                  rel_h=z(127, 64, dt=bf16), rel_w=z(127, 64, dt=bf16)), ["msam_global_attention16"],
          free={"q:0", "q:1"}, check=_attn_check,
          scalars=[("permuted q", {"q": z(1, 4096, 2, 64, dt=bf16).permute(0, 2, 1, 3)}, "q"), ("window table", {"rel_h": z(27, 64, dt=bf16)}, "rel_h")]),
    Entry("ops", "postprocess_masks", lambda: dict(low_res=z(2, 256, 256), input_size=(64, 64), original_size=(40, 50)), ["msam_postprocess_masks16"],
          free={"low_res:0"}, skip={"low_res:dtype": CONVERTED, "low_res:strides": CONVERTED}),
    Entry("ops", "rle_encode", lambda: dict(bits=z(2, 2, 50, dt=i32), height=40, width=50), ["msam_rle_run_counts", "msam_rle_encode"], free={"bits:0"},
          scalars=[("height of another mask", {"height": 70}, "bits")]),
    Entry("ops", "paint_label_image", lambda: dict(bits=z(2, 2, 50, dt=i32), order=z(2, dt=i64), height=40, width=50), ["msam_paint_label_image"],
          free={"bits:0", "order:0"}, skip={"order:dtype": CONVERTED, "order:strides": CONVERTED, "order:device": CONVERTED}),
    Entry("ops", "label_components", lambda: dict(seg=z(8, 8, dt=i32)), ["msam_label_components"], free={"seg:0", "seg:1"}, skip={"seg:strides": CONVERTED}),
    Entry("ops", "label_components_async", lambda: dict(seg=z(8, 8, dt=i32)), ["msam_label_components_async"], free={"seg:0", "seg:1"},
          skip={"seg:strides": CONVERTED}),
    Entry("ops", "box_nms", lambda: dict(boxes=z(3, 4), scores=z(3), iou_threshold=0.5), ["msam_box_nms"], free={"boxes:0"},
          skip={"boxes:dtype": CONVERTED, "boxes:strides": CONVERTED, "scores:dtype": CONVERTED, "scores:strides": CONVERTED},
          scalars=[("one box fewer", {"boxes": z(2, 4)}, "scores")]),
    Entry("ops", "box_nms_flags", lambda: dict(boxes=z(3, 4), scores=z(3), valid=z(3, dt=torch.bool), iou_threshold=0.5), ["msam_box_nms_valid"],
          free={"boxes:0"}, skip={"boxes:dtype": CONVERTED, "boxes:strides": CONVERTED, "scores:dtype": CONVERTED, "scores:strides": CONVERTED,
                                  "valid:strides": CONVERTED}),
    Entry("ops", "mask_nms", lambda: dict(bits=z(3, 2, 50, dt=i32), boxes_xyxy=z(3, 4), areas=z(3, dt=i32), scores=z(3), thresh=0.5, height=40),
          ["msam_mask_nms"], free={"bits:0", "bits:2"},
          skip={"bits:strides": CONVERTED, **{f"{n}:{k}": CONVERTED for n in ("boxes_xyxy", "areas", "scores") for k in ("dtype", "strides", "device")}}),
    Entry("ops", "wsgemm", _wsgemm_kw, ["msam_wsgemm_bf16"], free={"a:0", "w:0", "table:0", "table:1"}, blame={"a:size1": "w"},
          scalars=[("resid_rows > resid.shape[0]", {"resid_rows": 8}, "resid"), ("table_cols > table.shape[1]", {"table_cols": 192}, "table"),
                   ("table_cols no multiple of 4", {"table_cols": 6}, "table_cols"),
                   ("kv_split_tokens does not divide M", {"kv_split_tokens": 3, "out": None, "ln_mode": 0}, "kv_split_tokens")]),
    Entry("ops", "amg_generate_labels", lambda: dict(iou=z(3), stability=z(3), boxes=z(3, 4, dt=i32), area=z(3, dt=i32), bits=z(3, 2, 50, dt=i32),
                                                     shape=(40, 50), crop_box=(0, 0, 50, 40), pred_iou_thresh=0.5, stability_score_thresh=0.5, box_nms_thresh=0.5),
          ["msam_amg_generate_labels"], free={"iou:0"},
          skip={"bits:strides": CONVERTED, **{f"{n}:{k}": CONVERTED for n in ("iou", "stability", "boxes", "area") for k in ("dtype", "strides")}}),
    Entry("ops", "labels_from_masks", lambda: dict(bits=z(3, 2, 50, dt=i32), order=z(3, dt=i32), shape=(40, 50), k_dev=z(1, dt=i32)),
          ["msam_labels_from_masks"], free={"bits:0", "order:0"}, skip={"bits:strides": CONVERTED, "order:dtype": CONVERTED, "order:strides": CONVERTED}),
    Entry("ops", "paint_label_image_dev", lambda: dict(bits=z(3, 2, 50, dt=i32), order=z(3, dt=i32), k_dev=z(1, dt=i32), height=40, width=50),
          ["msam_paint_label_image_dev"], free={"bits:0", "order:0"}),
    Entry("ops", "slice_overlaps", lambda: dict(labels=z(2, 4, 4, dt=i32)), ["msam_slice_overlaps"], free={"labels:0", "labels:1", "labels:2"},
          skip={"labels:strides": CONVERTED}),
    Entry("ops", "objfeat_accumulate_batch", _objfeat_kw, ["msam_objfeat_gather", "msam_objfeat_accumulate", "msam_objfeat_finish"],
          free={"labels:0", "emb:0", "ids:0"},
          skip={"labels:rank": ANY_SHAPE, "emb:rank": ANY_SHAPE, "out:dtype": "fp32 and fp64 are both taken; an integer type is refused below"},
          scalars=[("embedding shorter than the unit", {"emb": z(256)}, "embedding"), ("out int64", {"out": z(2, 257, dt=i64)}, "out")]),
    Entry("ops", "objfeat_project", lambda: dict(labels=z(4, 4, dt=i64), ids=torch.ones(2, dtype=i64)), ["msam_objfeat_project"],
          free={"labels:0", "labels:1", "ids:0"}, skip={"labels:rank": ANY_SHAPE, "labels:strides": CONVERTED, "ids:strides": CONVERTED}),
    Entry("ops", "component_sizes", lambda: dict(roots=z(16, dt=i32)), ["msam_component_sizes"], free={"roots:0"}),
    Entry("ops", "decoder_image_layer", lambda: dict(xin=z(4096, 256, dt=f16), ktok=z(5, 128, dt=f16), vtok=z(5, 128, dt=f16), wo=z(256, 128, dt=f16), bo=z(256),
                                                     ln_w=z(256), ln_b=z(256), Nt=5, wq=z(128, 256, dt=f16), bq=z(128), peq=z(4096, 128), out=z(4096, 256, dt=f16)),
          ["msam_decoder_image_layer"], blame={"ktok:size0": "vtok"},
          scalars=[("rows beyond xin", {"rows": 8192, "out": None}, "xin"), ("more tokens than ktok holds", {"Nt": 6}, "ktok")]),
    Entry("ops", "t2i_fold_attention", lambda: dict(keys=z(2, 4096, 256, dt=f16), qtok=z(2, 5, 128, dt=f16), wk=z(128, 256, dt=f16), tabk=z(4096, 128, dt=f16),
                                                    wv=z(128, 256, dt=f16), bv=z(128)), ["msam_t2i_fold_attention"], free={"qtok:0", "qtok:1"}),
    Entry("ops", "i2t_fold_layer", lambda: dict(xin=z(2, 4096, 256, dt=f16), **_fold_kw(), tabq=z(4096, 128, dt=f16), ln_w=z(256), ln_b=z(256),
                                                out=z(2, 4096, 256, dt=f16)), ["msam_i2t_fold_layer"], free={"ktok:0", "ktok:1"},
          scalars=[("one prompt fewer in ktok / vtok", {"ktok": z(1, 5, 128, dt=f16), "vtok": z(1, 5, 128, dt=f16)}, "xin")]),
    Entry("ops", "i2t_fold_operands", _fold_kw, ["msam_i2t_fold_operands"], free={"ktok:0", "ktok:1"}),
    Entry("ops", "chain_prepare_tables", lambda: dict(src=z(4096, 256, dt=f16), q0=z(4096, 128, dt=f16), tabk=z(4096, 128, dt=f16), tabq1=z(4096, 128, dt=f16)),
          ["msam_chain_prepare_tables"]),
    Entry("ops", "i2t0_t2i_fused", lambda: dict(tables=blob(), operands0=blob(), ln0_w=z(256), ln0_b=z(256), qtok=z(2, 5, 128, dt=f16), wk=z(128, 256, dt=f16),
                                                wv=z(128, 256, dt=f16), bv=z(128)), ["msam_i2t0_t2i_fused"], free={"qtok:0", "qtok:1"},
          skip={"tables:strides": BLOB, "operands0:strides": BLOB}),
    Entry("ops", "chain_prepare_tables2", _chain2_kw, ["msam_chain_prepare_tables2"]),
    Entry("ops", "chain_prepare_tables2_cached", _chain2_kw, ["msam_chain_prepare_const2", "msam_chain_prepare_tables2_c"]),
    Entry("ops", "t2i_fold_values", lambda: dict(vtok0=z(2, 5, 128, dt=f16), tables2=blob()), ["msam_t2i_fold_values"], free={"vtok0:0", "vtok0:1"},
          skip={"tables2:strides": BLOB}),
    Entry("ops", "i2t_fold_operands_values", lambda: dict(**_fold_kw(), tables2=blob()), ["msam_i2t_fold_operands_values"], free={"ktok:0", "ktok:1"},
          skip={"tables2:strides": BLOB}),
    Entry("ops", "i2t0_t2i_fused_v2", lambda: dict(tables=blob(), tables2=blob(), operands0=blob(), mf=blob(), ln0_w=z(256), qtok=z(2, 5, 128, dt=f16),
                                                   wk=z(128, 256, dt=f16)), ["msam_i2t0_t2i_fused_v2"], free={"qtok:0", "qtok:1"},
          skip={f"{n}:strides": BLOB for n in ("tables", "tables2", "operands0", "mf")}),
    Entry("ops", "i2t01_fused", lambda: dict(tables=blob(), operands0=blob(), ln0_w=z(256), ln0_b=z(256), operands1=blob(), ln1_w=z(256), ln1_b=z(256), P=2, Nt=5),
          ["msam_i2t01_fused"], skip={f"{n}:strides": BLOB for n in ("tables", "operands0", "operands1")}),
    Entry("ops", "upscale_fused", lambda: dict(keys=z(2, 4096, 256, dt=f16), w1=z(256, 256, dt=f16), b1=z(256), ln_w=z(64), ln_b=z(64), w2=z(128, 64, dt=f16),
                                               b2=z(32), hyper=z(2, 4, 32), mask0=1, nmask=3), ["msam_upscale_fused_layout"], free={"keys:0"},
          scalars=[("masks beyond the four", {"mask0": 2}, "masks")]),
    Entry("ops", "uncrop_bits", lambda: dict(bits=z(2, 1, 20, dt=i32), crop_box=(5, 6, 25, 36), height=40, width=50), ["msam_uncrop_bits"], free={"bits:0"},
          skip={"bits:strides": CONVERTED}),
    Entry("strict", "weight_pairs", lambda: dict(w=torch.ones(4, 8), permute=False), ["msam_split16_prepare_pairs"], free={"w:0", "w:1"}),
    Entry("strict", "gemm", lambda: dict(a=z(6, 8), w=z(16, 8), bias=z(16), a2=z(3, 8), a2_rows=3, res=z(6, 16), out=z(6, 16)), ["msam_strict_gemm"],
          free={"a:0", "w:0", "a2:0"}, check=_sgemm_check, blame={"w:size1": "a"},
          scalars=[("a2_rows > a2.shape[0]", {"a2_rows": 4}, "a2"), ("res_rows > res.shape[0]", {"res_rows": 7}, "res"),
                   ("rows / lda beyond a", {"rows": 3, "lda": 24, "a_offset": 8, "out": None, "res": None}, "a")]),
    Entry("strict", "layer_norm", lambda: dict(x=z(6, 8), w=z(8), b=z(8), eps=1e-6, out=z(6, 8)), ["msam_strict_layernorm"], free={"x:0", "x:1"},
          skip={"x:rank": ANY_SHAPE, "out:rank": ANY_SHAPE}, scalars=[("rows beyond x", {"rows": 7, "dim": 8}, "x")]),
    Entry("strict", "attention", lambda: dict(q=z(6, 16), k=z(8, 16), v=z(8, 16), B=2, H=2, Nq=3, Nk=4, D=8, denom=2.0), ["msam_strict_attention"]),
    Entry("strict", "i2t_block", lambda: dict(keys=z(4096, 256), shared=False, pos=z(4096, 256), wq=(z(128, 256), z(128)), tok_k=z(5, 128), tok_v=z(5, 128),
                                              wo=(z(256, 128), z(256)), norm=(z(256), z(256), 1e-5), B=1, Tk=5, out=z(4096, 256)), ["msam_strict_i2t_block"],
          blame={"tok_k:size0": "tok_v"}),
]
BY_ID = {e.id: e for e in TABLE}

# public functions that hand no pointer to the library (the completeness test runs each under the recorder: zero calls)
EXEMPT = {
    "ops.quant_weight_fp8": ("torch arithmetic on the host, once per model", lambda f: f(torch.ones(4, 8))),
    "ops.rles_to_list": ("copies device RLE buffers to host lists", lambda f: f(z(0, dt=i32), z(1, dt=i64), 4, 4)),
    "ops.unpack_bits": ("torch shifts: a test / output helper", lambda f: f(z(1, 1, 4, dt=i32), 8)),
    "ops.to_blocked": ("a torch permutation", lambda f: f(z(4096, 32))),
    "ops.from_blocked": ("a torch permutation", lambda f: f(z(4096, 32))),
    "ops.upscale_centre_weights": ("torch arithmetic on the host, once per model", lambda f: f(torch.ones(256, 8), torch.ones(256))),
    "strict.decode_chunk": ("reads the free device memory", lambda f: f("cpu", False)),
    "strict.split_active": ("reads a thread-local flag", lambda f: f()),
    "strict.weight_scale": ("torch reduction, cached per weight", lambda f: f(torch.ones(2, 2))),
    "strict.forget_scales": ("clears two caches", lambda f: f()),
}
