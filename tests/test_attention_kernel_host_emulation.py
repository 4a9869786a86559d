"""window_attention_kernel and global_attention_kernel (csrc/attention.hip) executed on the CPU behind tests/hip_host_shim.py (the lanes of
a wave as host contexts, the MFMA in its register layout), in all four builds of each - stored head_dim 64 / 96 (80 real channels) times
bf16 / fp16 -: staging of K / V^T with the bias-only padding tokens of the 70 x 70 padded grid, rel-pos terms by MFMA, masked softmax,
P V - against the fp64 restatement of SAM's attention with decomposed relative position bias on the same 16-bit q / k / v and within its
elementwise rounding bound (tests/attention_ref.py).  B = 2 images of 3 heads, a chosen few workgroups of each kernel, so that the
decomposition of the workgroup index is part of what is checked.  The device runs of the same kernels: tests/test_gpu_attention.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

import attention_ref as R
from hip_host_shim import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "micro_sam_amd", "csrc", "attention.hip")

# The workgroups to run are LISTED (wgs[n]): the shim's launch_grid walks blockIdx.y = 0 .. n - 1 with blockIdx.x = 0, and every lane
# sets blockIdx.x = wgs[blockIdx.y] before it enters the kernel (the kernels read blockIdx.x only).
ENTRY = r"""
#define EMU_GO(kern_, ...)                                                                              \
    do {                                                                                               \
        if (hd == 64 && f16) launch_grid(1, n, [=] { blockIdx.x = wgs[blockIdx.y]; kern_<64, true>(__VA_ARGS__); });        \
        else if (hd == 64) launch_grid(1, n, [=] { blockIdx.x = wgs[blockIdx.y]; kern_<64, false>(__VA_ARGS__); });         \
        else if (f16) launch_grid(1, n, [=] { blockIdx.x = wgs[blockIdx.y]; kern_<96, true>(__VA_ARGS__); });               \
        else launch_grid(1, n, [=] { blockIdx.x = wgs[blockIdx.y]; kern_<96, false>(__VA_ARGS__); });                       \
    } while (0)
extern "C" void emu_global_attention(int f16, int hd, const u16* q, const u16* k, const u16* v, const u16* relh, const u16* relw,
                                     const int* wgs, int n, int heads, float scale, u16* out) {
    EMU_GO(global_attention_kernel, q, k, v, relh, relw, heads, scale, out);     // workgroup = (image, head, 128 queries = two image rows)
}
extern "C" void emu_window_attention(int f16, int hd, const u16* q, const u16* k, const u16* v, const u16* relh, const u16* relw,
                                     const float* bias, const int* wgs, int n, int heads, float scale, u16* out) {
    EMU_GO(window_attention_kernel, q, k, v, relh, relw, bias, heads, scale, out);        // workgroup = (image, window, head)
}
"""


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    text = open(SRC).read()
    start = text.index("constexpr int TOK = 4096;")
    end = text.index("}  // namespace", start)
    body = text[start:end]
    assert "window_attention_kernel" in body and "global_attention_kernel" in body
    # the transposing LDS read is a clang builtin on an address-space pointer: the shim's restatement takes its place
    a = body.index("typedef short gs16x4_t")
    b = body.index("template <int HD, bool F16 = false>", a)
    body = body[:a] + "static inline uint2 g_tr16(const unsigned char* p) { return ds_read_tr16_b64_emu(p); }\n" + body[b:]
    lib = build(str(tmp_path_factory.mktemp("emu_attn")), "attn", body, ENTRY)
    lib.emu_window_attention.argtypes = [ctypes.c_int] * 2 + [ctypes.c_void_p] * 7 + [ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_void_p]
    lib.emu_global_attention.argtypes = [ctypes.c_int] * 2 + [ctypes.c_void_p] * 6 + [ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_void_p]
    return lib


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _bits(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16).copy()


B, HEADS = 2, 3
BUILDS = [(hs, dtype) for hs in (64, 96) for dtype in (torch.bfloat16, torch.float16)]
BUILD_IDS = [f"hd{hs}-{'fp16' if dtype == torch.float16 else 'bf16'}" for hs, dtype in BUILDS]


def _run(emu, kind, inp, wgs):
    """The listed workgroups of one kernel on ``inp`` -> the [B * 4096, heads * hs] output as fp64 (zero where nothing was written)."""
    dtype, hs = inp["q"].dtype, inp["q"].shape[-1]
    out = np.zeros((B * R.TOK, HEADS * hs), np.uint16)
    ops = [_bits(inp[n]) for n in ("q", "k", "v", "rel_h", "rel_w")]
    wa = np.asarray(wgs, np.int32)
    head = [int(dtype == torch.float16), hs] + [_ptr(a) for a in ops]
    tail = [_ptr(wa), len(wa), HEADS, ctypes.c_float(inp["scale"]), _ptr(out)]
    if kind == "window":
        ba = inp["qkv_bias"].numpy().copy()
        emu.emu_window_attention(*head, _ptr(ba), *tail)
    else:
        emu.emu_global_attention(*head, *tail)
    return torch.from_numpy(out.view(np.int16)).view(dtype).double()


def _check(got, ref, bound, ran):
    """``ran``: bool mask of the elements the listed workgroups own.  Those are within the bound, the rest was not touched."""
    assert bool(torch.isfinite(got).all())
    assert float(got[~ran].abs().max()) == 0.0
    ratio = ((got - ref).abs()[ran & (bound > 0)] / bound[ran & (bound > 0)]).max().item()
    print(f"max |got - ref| / bound = {ratio:.3f}")
    assert bool(((got - ref).abs() <= bound)[ran].all()), ratio


@pytest.mark.parametrize("hs,dtype", BUILDS, ids=BUILD_IDS)
def test_window_attention_kernel_source_on_the_cpu(emu, hs, dtype):
    """Every one of the 25 windows once, window w of image w % 2 and head w % 3 (all six (image, head) pairs occur): interior windows,
    the edge windows with 6 of 14 bias-only rows / columns and the corner window, with a qkv bias of std 1 (generator "padding")."""
    inp = R.make_inputs("window", "padding", dtype, hs, B, HEADS, seed=3)
    wgs = [((w % 2) * 25 + w) * HEADS + w % 3 for w in range(25)]
    got = _run(emu, "window", inp, wgs)
    ref, bound = R.attention_ref("window", inp)
    ran = torch.zeros(B, 70, 70, HEADS, hs, dtype=torch.bool)
    for w in range(25):
        ran[w % 2, (w // 5) * 14:(w // 5 + 1) * 14, (w % 5) * 14:(w % 5 + 1) * 14, w % 3] = True
    _check(got, ref, bound, ran[:, :64, :64].reshape(B * R.TOK, HEADS * hs))


@pytest.mark.parametrize("hs,dtype", BUILDS, ids=BUILD_IDS)
def test_global_attention_kernel_source_on_the_cpu(emu, hs, dtype):
    """Global attention (4096 keys): rel_h / rel_w tables by MFMA in the prologue, 128 key tiles with the base-2 online softmax on
    float pairs, accumulators rescaled only when the running maximum moves, V^T through the transposing LDS read (here: the shim's
    restatement of it).  Five of the B * heads * 32 workgroups: image rows 0-1 and 62-63 (rel-pos table rows 0 and 126) of different
    (image, head) pairs and one in between.  Generator "peaked": the running maximum moves between tiles for some queries and stays put
    for others (both sides of the conditional rescale)."""
    inp = R.make_inputs("global", "peaked", dtype, hs, B, HEADS, seed=11)
    picks = [(0, 0, 0), (0, 1, 31), (1, 2, 0), (1, 0, 31), (1, 1, 17)]                     # (image, head, pair of image rows)
    got = _run(emu, "global", inp, [(b * HEADS + h) * 32 + qp for b, h, qp in picks])
    ref, bound = R.attention_ref("global", inp, pairs=[(b, h) for b, h, _ in picks])
    ran = torch.zeros(B, 32, 128, HEADS, hs, dtype=torch.bool)
    for b, h, qp in picks:
        ran[b, qp, :, h] = True
    _check(got, ref, bound, ran.reshape(B * R.TOK, HEADS * hs))
