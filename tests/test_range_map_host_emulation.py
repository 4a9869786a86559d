"""The range map of the low-res logits on the CPU, both ends of it (no GPU):

* up_fused_kernel's map instantiations (csrc/upfused.hip, CEN bit 1) behind tests/hip_host_shim.py: the logits are those of the
  launch without the map bit for bit, the map is the {min, max} of every 64-pixel segment of every low-res row of exactly those
  logits, every entry is written and nothing outside the map is;
* postprocess_range_kernel (csrc/postprocess.hip) behind the shim of tests/test_postprocess_kernel_host_emulation.py against
  postprocess_kernel<false, false, float> on the same inputs: counts, boxes and bit words equal, with the true map and with a looser one,
  on masks built around every edge of the settling rule (segment borders, the row halo, the clamps, the 0.01 margin, |value| >= 8192)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import test_postprocess_kernel_host_emulation as PP
import test_upfused_kernel_host_emulation as UF
from hip_host_shim import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ------------------------------------------------------------------------------------------------------------- up_fused_kernel

UP_ENTRY = r"""
extern "C" void emu_up_range(int variant, const u16* keys, int blocked, int P, const u16* w1, const float* b1, const float* lnw, const float* lnb,
                             float eps, const u16* w2, const float* b2, const float* hyper, int hyper_ld, int mask0, int nmask, float* out,
                             float* range) {
    UpArgs a{};
    a.keys = keys; a.w1 = w1; a.b1 = b1; a.lnw = lnw; a.lnb = lnb; a.eps = eps; a.w2 = w2; a.b2 = b2; a.hyper = hyper; a.hyper_ld = hyper_ld;
    a.mask0 = mask0; a.nmask = nmask; a.KS = 2; a.nitems = P * 2; a.out = out; a.blocked = blocked; a.range = range;
    // 3 workgroups over 2 P work items: uneven shares
    if (variant == 0) launch_grid(3, 1, [=] { up_fused_kernel<1, 1>(a); });                 // packed-fp16 GELUs, plain weights
    else if (variant == 1) launch_grid(3, 1, [=] { up_fused_kernel<1, 1, 0, 2>(a); });      //   + range map
    else if (variant == 2) launch_grid(3, 1, [=] { up_fused_kernel<1, 0, 0, 1>(a); });      // fp32 GELUs, centred weights
    else launch_grid(3, 1, [=] { up_fused_kernel<1, 0, 0, 3>(a); });                        //   + range map
}
"""


@pytest.fixture(scope="module")
def up_emu(tmp_path_factory):
    common = open(os.path.join(ROOT, "micro_sam_amd", "csrc", "common.h")).read()
    a = common.index("MSAM_DEVINL float relu1(float x)")
    gelu = common[a:common.index("// round-to-nearest-even fp32 -> packed fp16", a)]
    text = open(os.path.join(ROOT, "micro_sam_amd", "csrc", "upfused.hip")).read()
    s0 = text.index("constexpr int SUB_BYTES = TK * 64 + 64")
    s1 = text.index("// erf-GELU of two values in PACKED fp16 arithmetic")
    k0 = text.index("template <int UF_PRIO, int G16, int LN2P = 0, int CEN = 0>")
    k1 = text.index("}  // namespace", k0)
    lib = build(str(tmp_path_factory.mktemp("emu_up_range")), "up_range", UF.DEC + gelu + text[s0:s1] + text[k0:k1], UP_ENTRY)
    vp, i = ctypes.c_void_p, ctypes.c_int
    lib.emu_up_range.argtypes = [i, vp, i, i, vp, vp, vp, vp, ctypes.c_float, vp, vp, vp, i, i, i, vp, vp]
    return lib


@pytest.mark.parametrize("base,blocked,mask0,nmask", [(0, 0, 1, 3), (2, 1, 0, 1)])
def test_up_fused_range_map_source_on_the_cpu(up_emu, base, blocked, mask0, nmask):
    g = torch.Generator().manual_seed(21 + base + blocked)
    P = 2                                              # four half-prompt items over three workgroups
    keys = UF._h(torch.randn(P, 4096, 256, generator=g))
    w1 = UF._h(torch.randn(256, 256, generator=g) / 16); b1 = torch.randn(64, generator=g).repeat(4)
    lw, lb = torch.randn(64, generator=g) * 0.2 + 1, torch.randn(64, generator=g) * 0.3
    w2 = UF._h(torch.randn(128, 64, generator=g) / 8); b2 = torch.randn(32, generator=g)
    hyper = torch.randn(P, 4, 128, generator=g)
    if base == 2:
        w1, b1 = UF._centre(w1, b1)
    stream = keys.reshape(P, 256, 16, 8, 4, 8).permute(0, 1, 3, 4, 2, 5).contiguous() if blocked else keys
    f32 = lambda t: t.numpy().astype(np.float32).copy()
    arrs = [UF._bits(stream), UF._bits(w1), f32(b1), f32(lw), f32(lb), UF._bits(w2), f32(b2), f32(hyper)]
    p = [UF._ptr(a) for a in arrs]

    def run(variant, out, rng):
        up_emu.emu_up_range(variant, p[0], blocked, P, p[1], p[2], p[3], p[4], 1e-6, p[5], p[6], p[7], 128, mask0, nmask, UF._ptr(out),
                            UF._ptr(rng) if rng is not None else None)

    plain = np.full((P, nmask, 256, 256), np.nan, np.float32)
    run(base, plain, None)
    assert np.isfinite(plain).all() and plain.std() > 0
    SENT = np.float32(-12345.5)
    guard = 64                                          # floats in front of and behind the map: must stay untouched
    buf = np.full(guard + P * nmask * 256 * 4 * 2 + guard, SENT, np.float32)
    rng = buf[guard:-guard]
    out = np.full((P, nmask, 256, 256), np.nan, np.float32)
    run(base + 1, out, rng)
    assert np.array_equal(out.view(np.uint32), plain.view(np.uint32)), "the map instantiation changed the logits"
    assert (buf[:guard] == SENT).all() and (buf[-guard:] == SENT).all(), "a store outside the map"
    assert (rng != SENT).all(), "map entries that were never written"
    seg = out.reshape(P, nmask, 256, 4, 64)
    want = np.stack([seg.min(-1), seg.max(-1)], -1)
    assert np.array_equal(rng.reshape(P, nmask, 256, 4, 2), want)


# ------------------------------------------------------------------------------------------------------- postprocess_range_kernel

PP_EXTRA = r"""
extern "C" void emu_postprocess_range(const float* low, const float* range, float thr, float off, int* counts, int* boxes, uint32_t* bits, int N) {
    for (int n = 0; n < N; ++n) for (int bx = 0; bx < 4; ++bx) {
        std::barrier<> b0(64), b1(64), b2(64), b3(64), bb(256);
        wave_bar[0] = &b0; wave_bar[1] = &b1; wave_bar[2] = &b2; wave_bar[3] = &b3; block_bar = &bb;
        std::vector<std::thread> ts;
        for (int tx = 0; tx < 256; ++tx)
            ts.emplace_back([=] {
                threadIdx = {tx, 0, 0}; blockIdx = {bx, n, 0};
                postprocess_range_kernel(low, range, thr, off, counts, boxes, bits);
            });
        for (auto& t : ts) t.join();
    }
}
extern "C" void emu_postprocess_x4(const float* low, float thr, float off, int* counts, int* boxes, uint32_t* bits, int N) {
    run<false, false>(low, 1024, 1024, 1024, 1024, thr, off, counts, boxes, bits, nullptr, N);
}
"""


def _pp_source():
    text = open(PP.SRC).read()
    body = text[text.index("struct Axis {"):text.index("// ---------------------------------------------------------------------------------------------- RLE")]
    assert "postprocess_range_kernel" in body
    return body


def _pp_build(d, body):
    cpp, so = os.path.join(d, "pp.cpp"), os.path.join(d, "pp.so")
    open(cpp, "w").write(PP.SHIM % body + PP_EXTRA)
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-pthread", "-Wno-unknown-pragmas", cpp, "-o", so])
    lib = ctypes.CDLL(so)
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.emu_postprocess_range.argtypes = [vp, vp, f, f, vp, vp, vp, i]
    lib.emu_postprocess_x4.argtypes = [vp, f, f, vp, vp, vp, i]
    return lib


@pytest.fixture(scope="module")
def pp_emu(tmp_path_factory):
    return _pp_build(tmp_path_factory.mktemp("emu_pp_range"), _pp_source())


# (low-res row, low-res column, (word, output column) set through the ROW HALO only, (word, output column) set through the NEIGHBOUR SEGMENT only)
EDGE_MASK = 2
EDGE_FEATURES = ((8 * 5 - 1, 63, (5, 253), (4, 256)),            # last row above word 5; last column of segment 0, seen from block 1
                 (8 * 11 + 8, 64, (11, 257), (12, 255)),         # first row below word 11; first column of segment 1, seen from block 0
                 (8 * 17 - 1, 128, (17, 513), (16, 511)),        # ... of segment 2, seen from block 1
                 (8 * 29 + 8, 191, (29, 765), (30, 768)))        # ... last column of segment 2, seen from block 3


def edge_words_are_set(bits) -> bool:
    """The words of mask EDGE_MASK that only the row halo / only the neighbour segment reaches are non-zero in `bits` [N,32,1024]: the
    reference must say so, or the case shows nothing."""
    return all(int(bits[EDGE_MASK, yw, x]) != 0 for f in EDGE_FEATURES for (yw, x) in f[2:])


def crafted_masks(thr: float, off: float) -> np.ndarray:
    """256 x 256 low-res masks: a constant background plus features at every edge of the settling rule (shared with the device test)."""
    f = np.float32
    far = f(20.0)
    ms = []
    ms.append(np.full((256, 256), thr - far, f))                         # every word settled zero
    ms.append(np.full((256, 256), thr + far, f))                         # every word settled one: counts 1024^2, full box
    # EDGE_FEATURES (mask EDGE_MASK): pixels of thr + 100 at a segment border's two sides, each in the first row of a word's halo above it
    # or the last below it.  Through the bilinear weight 0.375 such a pixel still lifts the nearest pixels of the NEIGHBOURING block
    # (0.375 * 100 - 0.625 * 20 = 25 above thr) and of the neighbouring word over all three thresholds, while that block's own
    # segment and that word's own eight rows hold the background only: a footprint without the neighbour segment or without the halo
    # rows settles them as zero.  (Far apart: every pixel has its own words and blocks.)
    m = np.full((256, 256), thr - far, f)
    for (r, c, _, _) in EDGE_FEATURES:
        m[r, c] = thr + f(100.0)
    ms.append(m)
    m = np.full((256, 256), thr - far, f)
    for (r, c) in ((0, 0), (0, 255), (255, 0), (255, 255)):              # the clamps
        m[r, c] = thr + f(100.0)
    ms.append(m)
    ms.append(np.full((256, 256), f(thr + off + 0.005), f))               # inside the 0.01 margin: not settled
    ms.append(np.full((256, 256), f(thr - off - 0.005), f))
    m = np.full((256, 256), thr + far, f); m[100, 70] = f(8192.0); m[60:70, 60:70] = thr - far; ms.append(m)     # |value| >= 8192: not settled; a hole
    m = np.full((256, 256), thr - far, f); m[9, 200] = f(-9000.0); ms.append(m)
    yy, xx = np.meshgrid(np.arange(256, dtype=f), np.arange(256, dtype=f), indexing="ij")
    m = np.full((256, 256), -np.inf, f)
    for (cy, cx, rad) in ((64.0, 64.0, 30.0), (127.5, 191.5, 40.0), (8.0, 250.0, 12.0)):      # smooth blobs over word and block borders
        m = np.maximum(m, (thr + (f(1.0) - np.sqrt((yy - f(cy)) ** 2 + (xx - f(cx)) ** 2) / f(rad)) * f(12.0)).astype(f))
    ms.append(m)
    return np.stack(ms)


def true_map(low: np.ndarray) -> np.ndarray:
    seg = low.reshape(low.shape[0], 256, 4, 64)
    return np.ascontiguousarray(np.stack([seg.min(-1), seg.max(-1)], -1))


def _run_pp(lib, low, rng, thr, off):
    N = low.shape[0]
    counts = np.zeros((N, 3), np.int32)
    boxes = np.tile(np.array([0x7fffffff, 0x7fffffff, -1, -1], np.int32), (N, 1))
    bits = np.full((N, 32, 1024), 0x5a5a5a5a, np.uint32)
    if rng is None:
        lib.emu_postprocess_x4(PP._ptr(low), thr, off, PP._ptr(counts), PP._ptr(boxes), PP._ptr(bits), N)
    else:
        lib.emu_postprocess_range(PP._ptr(low), PP._ptr(rng), thr, off, PP._ptr(counts), PP._ptr(boxes), PP._ptr(bits), N)
    return counts, boxes, bits


@pytest.mark.parametrize("thr,off", [(0.0, 1.0), (0.75, 0.0)])
def test_postprocess_range_kernel_source_on_the_cpu(pp_emu, thr, off):
    low = crafted_masks(thr, off)
    ref = _run_pp(pp_emu, low, None, thr, off)
    assert ref[0][1].tolist() == [1024 * 1024] * 3 and ref[1][1].tolist() == [0, 0, 1023, 1023]      # the settled-one mask
    assert ref[0][0].tolist() == [0, 0, 0]
    assert edge_words_are_set(ref[2])
    rng = true_map(low)
    loose = rng.copy()
    loose[..., 0] -= np.float32(0.75); loose[..., 1] += np.float32(0.75)
    loose[::2, 40:48, :, 0] = -np.inf; loose[1::2, 200:, 2:, 1] = np.inf        # (a looser map may only settle fewer words)
    loose[0, 100:104, 1, 0] = np.nan; loose[1, 17, 2, 1] = np.nan               # (a NaN entry leaves its words unsettled)
    for name, m in (("true map", rng), ("loose map", loose)):
        got = _run_pp(pp_emu, low, m, thr, off)
        for what, a, b in zip(("counts", "boxes", "bits"), got, ref):
            assert np.array_equal(a, b), (name, what, np.argwhere(a != b)[:5].tolist())


@pytest.mark.parametrize("what,old,new", [
    ("no neighbour segment", "for (int s = max(bx - 1, 0); s <= min(bx + 1, 3); ++s) {", "for (int s = bx; s <= bx; ++s) {"),
    ("no row halo", "for (int r = max(8 * yw - 1, 0); r <= min(8 * yw + 8, 255); ++r)", "for (int r = 8 * yw; r <= 8 * yw + 7; ++r)")])
def test_the_edge_mask_tells_a_footprint_that_is_too_small(pp_emu, tmp_path, what, old, new):
    """The crafted edge mask does its job: the kernel source with the footprint cut down to the block's own segment, or to the word's own
    eight rows, gives wrong bits on it (and the unmodified source does not)."""
    body = _pp_source()
    kern = body.index("void postprocess_range_kernel(")
    assert body.count(old, kern) == 1, what
    mutant = _pp_build(str(tmp_path), body[:kern] + body[kern:].replace(old, new))
    low = crafted_masks(0.0, 1.0)[:EDGE_MASK + 1]
    ref = _run_pp(pp_emu, low, None, 0.0, 1.0)
    assert edge_words_are_set(ref[2])
    assert np.array_equal(_run_pp(pp_emu, low, true_map(low), 0.0, 1.0)[2], ref[2])
    bad = _run_pp(mutant, low, true_map(low), 0.0, 1.0)
    assert not np.array_equal(bad[2][EDGE_MASK], ref[2][EDGE_MASK]), what
    assert not edge_words_are_set(bad[2])
