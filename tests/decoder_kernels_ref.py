"""float64 references, elementwise rounding bounds, input families, the case table and the call layer for the 13 small kernels of
csrc/decoder.hip: prompt encoding (``sparse_embed_kernel``, ``prompt_tokens_kernel``, ``dense_pe_kernel``, ``mask_src_kernel``), the
token-side attention (``token_self_attn_kernel``, ``t2i_attn_kernel``, ``t2i_shared_kernel<4 | 8 | 16>``) and the source stream
(``src_prepare_kernel``, ``dense_src_kernel``, ``tokens_from_sparse_kernel``, the keys form of ``mask_src_kernel``, ``add_cast_kernel``,
``add_cast2_kernel``).  No fixtures and no kernel text: the references are written from upstream's formulation (segment_anything's
PromptEncoder / PositionEmbeddingRandom / Attention) in numpy / torch float64.  tests/test_decoder_kernels_host.py runs the table (and
mutated copies of the source) on the CPU, tests/test_gpu_decoder_kernels.py on the device; both go through ``Backend``.

u = 2^-24 (fp32), u16 = 2^-11 / 2^-8 the unit roundoff of the decoder's 16-bit type (fp16 / bf16), SUB = 2^-25 the absolute rounding
error below fp16's normal range (0 for bf16).  Every bound is computed from the inputs and the kernels' operation counts, never from a
kernel's output.

CONSTANTS FOR THE DEVICE INTRINSICS, stated before any measurement:
* ``sinf`` / ``cosf``: E_SINCOS = 4 ulp.  They are the OpenCL math library's f32 functions (OCML), which is built to the OpenCL
  full-profile accuracy table: sin, cos <= 4 ulp on the whole range (the Payne-Hanek reduction is part of that contract).
* ``erff``: E_ERF = 16 ulp, the same table's figure for erf.
* ``__builtin_amdgcn_exp2f`` is v_exp_f32: E_EXP2 = 1 ulp, the ISA guide's statement for the instruction.
* ``__expf(x)`` is v_exp_f32(x log2 e): the instruction's 1 ulp, the product and the rounded constant: a log error of u (2 |x| + 2);
  the subtraction that forms x is one more rounding of x: LOGERR_EXP(x) = u (3 |x| + 2) (tests/decoder_fold_ref.py uses the same model).
  The attention outputs are 16 bit, so no float64 value isolates ``__expf`` here; tests/train_attention_ref.py measured it on the device
  through fp32 outputs (E_MEASURED there).  A result below 2^-126 is flushed to zero: FLOOR absorbs it.
An ulp of a result r is at most 2^-23 |r|.  The GPU test measures sinf, cosf, erff and v_exp_f32 in isolation (E_MEASURED below).

FOURIER FEATURES (sparse rows, prompt tokens, dense grid).  Reference from the fp32 inputs in float64:
    c = (p + 0.5) / 1024 (dense grid: (t + 0.5) / 64),  x = 2 c - 1,  v = fp32(2 pi) (x G0 + y G1),  row = [sin v | cos v] (+ embedding).
The kernel rounds p + 0.5 (u |x + 1| of x; the division by 1024 and the doubling are exact), the subtraction (u |x|), the two products
(u |a|, u |b| with a = x G0, b = y G1 - one of them is absorbed when the compiler contracts x G0 + y G1 into an FMA, so the count holds
with and without contraction), their sum (u |a + b|) and the product with 2 pi (u |v|):
    dv = 2 pi (|G0| u (|x + 1| + |x|) + |G1| u (|y + 1| + |y|) + u (|a| + |b|) + u |a + b|) + u |v|    (<= 6 u 2 pi (|a| + |b|) + 2 u 2 pi (|G0| + |G1|)),
then |sin' - sin| <= dv + E_SINCOS 2^-23 |sin| and the embedding add rounds once more (u |row|).  (1 + 2^-10) covers second order.

MASK DOWN-SCALING (``mask_ref``): conv 2x2/2 (1 -> 4) -> LayerNorm2d(1e-6) -> GELU -> conv 2x2/2 (4 -> 16) -> LayerNorm2d -> GELU -> conv 1x1
(16 -> 256), in float64, in both GELU forms: ``exact`` = 0.5 z (1 + erf(z / sqrt 2)); default = max(z, 0) - |z| 2^q(|z|) with the cubic q
of tests/upscale_fused_ref.py (``CUBIC``) evaluated in float64 - that approximant is the default mode's specification.  The bound is
carried stage by stage, per pixel: a convolution of n taps (n FMAs from the bias) adds n u of its absolute sum (n + 1 behind a rounded
input) to |w| * (error of its input); through a
LayerNorm over n channels with input error E (Ebar = mean E, E2 = rms E, the kernel's own roundings added to E first: u (n - 1) mean |a|
for the mean's chain of adds, 2 u |dev| for the centring and the square) as in tests/decoder_fold_ref.py, without linearising:
    |z' - z| <= |w| ((E + Ebar) / (sig - E2) + |dev| E2 / (sig (sig - E2))) + (n + 8) u |w| |dev| / sig + u |z|,
so 1 / sig (``rstd``) amplifies what is in front of it pixel by pixel; the GELUs have slope <= 1.13 and add their own evaluation error
(the erf form: the rounded argument, E_ERF ulp of erf, the sum and the two products; the cubic form: 3 FMAs of the Horner chain through
ln 2 |z| 2^q, E_EXP2 ulp of the exponential, the final FMA).  The keys form adds the fp32 roundings of embedding + no_mask, c3_b - no_mask
and the final sum, and ONE 16-bit rounding: u16 |value| + SUB.

ATTENTION (``self_attn_ref``, ``t2i_ref``): softmax(q k^T scale) v per head in float64 on the values of the 16-bit operands; 8 heads x 32
channels and scale 1 / sqrt 32 over the <= 16 tokens of a prompt, 8 heads x 16 and scale 1/4 over the 4096 image tokens.  The bound is
the model of tests/decoder_fold_ref.py.  Scores: products of 16-bit values are exact in fp32, their sum passes <= 32 roundings (one MFMA
of K = 32, or 32 chained adds) + 2 for the self-attention's rounded scale: n_s u Sabs.  Every weight passes its own ``__expf``, the
rescales alpha = exp(m_old - m_new) of the later 32-key steps (their arguments telescope to <= the score range R; <= 32 of them per
wave) and the merge's exp(m_w - M): a log error eps = n_s u max Sabs + u (9 R + 70) (self attention: one exp, u (3 R + 2)).  The kernel's
weights are then P'_j = P_j e^(d_j) / sum_k P_k e^(d_k), |d| <= eps, and because the differences sum to zero
    |out' - out| <= (e^(2 eps) - 1) (P @ |V - out|) <= (e^(2 eps) - 1) sqrt(P @ V^2 - out^2)          (Jensen).
Token->image only: the un-normalised probabilities exp(s - m_running) are rounded to 16 bit before the PV product while l sums the
unrounded ones: u16 e^(2 eps) (P @ |V|); a probability that may lie below fp16's normal range (exp(s_j - max) < 2^-14: m_running <= max)
errs by <= SUB absolutely, at most SUB |V_j| in the output because l >= 1 relative to the final maximum: SUB (sub-mask @ |V|) - the
subnormal step of fp16 and the flush to zero below 2^-25.  fp32 accumulation: a term of O passes <= 32 roundings in its MFMA, two per
later step (rescale, next MFMA's add) and the merge (product, 3 adds, reciprocal, product): 102 u; l 80 u: ACC_T2I = 200 u (P @ |V|);
self attention 64 u.  One final 16-bit rounding: u16 |got| + SUB with |got| <= |out| + everything above.

EXACT FAMILIES (bit for bit):
* ``uniform``: q = 0 and small integer v: every probability is exactly 1, l the key count, O an integer below 2^24; the output is the
  exact mean rounded once (4096 keys: the division is exact; self attention: v is built so that the mean is an integer, which 1 ulp
  of the fp32 reciprocal cannot move across a 16-bit rounding boundary).  The mean differs per (prompt, head, channel).
* ``onehot``: one key pi(p, head, token) leads by >= 32 in the score, so every other probability is < 2^-46 - zero after its 16-bit
  rounding, and below half an ulp of the non-zero integer v values in fp32 even unrounded (self attention, the rescaled remains of a
  wave's earlier maxima, the other waves in the merge): the output is v[pi] bit for bit.  Token->image: keys are the lifted lattice
  points (a_j, -|a_j|^2 / 2), a_j in {0, 2, .., 14}^4 (4096 of them; a prompt-specific permutation for per-prompt K / V), q = 64 (a_pi, 1):
  score = 16 (|a_pi|^2 - |a_pi - a_j|^2) / 2, integers below 2^24, exact in fp32.  Two variants: pi distinct for every (prompt, head,
  token) (an odd multiplier mod 4096), and pi on the edges of the 32-key steps and of the four waves' key quarters.  fp16 only (bf16
  has no 16-bit rounding to zero at e^-32).
* label -1 and padding rows equal ``not_a_point_embed``; a label outside {-1, 0, 1} gives the bits of the same point under label 0 with
  a zeroed label-0 embedding; ``tokens_from_sparse`` copies; ``add_cast`` / ``add_cast2`` / ``src_prepare`` / ``dense_src`` = round16 of the
  fp32 sum (numpy forms the IEEE fp32 sum, torch rounds it to nearest even).
BOUNDED FAMILIES: ``diffuse`` (scores about N(0, 1)); ``first`` / ``rising`` / ``needle``: one q / k channel carries a ramp over the keys
worth +-40 in the score - descending (the running maximum never moves), ascending (it moves at every 32-key step of every wave; the
early keys' probabilities pass through fp16's subnormal range to zero), or a single key 30 above the rest among the last 32 keys of
the last wave.  Self attention has no key steps: ``diffuse`` and ``peaked`` (scores about N(0, 36)).

THE CASE TABLE takes the smallest values that reach each branch (the key count 4096 is fixed by the kernels): self attention
Nt in (1, 5, 7, 8, 9, 15, 16) x P in (1, 3); ``t2i_attn_kernel`` Nt in (9, 12, 16) x shared / per-prompt K, V x P in (1, 3);
``t2i_shared_kernel<G>`` G in (4, 8, 16) x Nt in (5, 7, 8) x P in (1, G - 1, G, G + 1, 2 G + 1): odd and even tails, a tail with a
half-filled score tile, tiles that must not be merged; the same prompts in a launch of P - 1 must give equal bits.
"""
import ctypes
import math

import numpy as np
import torch

T, C, CI, H = 4096, 256, 128, 8
F32 = 2.0 ** -24
ULP = 2.0 ** -23                          # an ulp of a result r is at most ULP |r|
U16 = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
SUB16 = {torch.float16: 2.0 ** -25, torch.bfloat16: 0.0}
E_SINCOS, E_ERF, E_EXP2 = 4.0, 16.0, 1.0
# Measured on an MI355X by test_intrinsics_are_within_the_constant_the_bounds_use, in ulp of the result; never fitted to a kernel's output
# (sinf / cosf over 11520 arguments up to 2 pi * 190; erff over 96 arguments in (0, 9), after the two roundings around it; v_exp_f32 over 96
# arguments down to about 2^-70, after the product's rounding).  On the host emulation (glibc): 0.56, 0.55, 0.0, 0.20.  The constants hold and stay.
E_MEASURED = {"sinf": 1.342, "cosf": 1.337, "erff": 0.0, "v_exp_f32": 0.334}
FLOOR = 2.0 ** -100
SECOND = 1.0 + 2.0 ** -10
GELU_SLOPE = 1.13
CUBIC = tuple(float(np.float32(c)) for c in (-0.0248758, -0.49884797, -1.12922424, -1.00353579))      # c3 .. c0 (tests/upscale_fused_ref.py)
LN_EPS = 1e-6
PATTERN16 = 0x7FC1                        # guard zones and output prefill: a NaN as fp16, as bf16 and (twice) as fp32
GUARD = 16384                             # bytes in front of and behind every array of a call

SELF_NT, SELF_P = (1, 5, 7, 8, 9, 15, 16), (1, 3)
SELF_FAMILIES = ("uniform", "onehot", "diffuse", "peaked")
T2I_NT, T2I_P = (9, 12, 16), (1, 3)
SHARED_G, SHARED_NT = (4, 8, 16), (5, 7, 8)
T2I_FAMILIES = ("uniform", "onehot:0", "onehot:1", "diffuse", "first", "rising", "needle")
EDGE_KEYS = (0, 31, 32, 1023, 1024, 2047, 2048, 3071, 3072, 4063, 4064, 4095)
LABELS = (-1, 0, 1, 2, 3, 7)
POINTS = ((-0.5, -0.5), (0.0, 0.0), (1023.0, 1023.0), (1023.5, 1023.5), (511.5, 511.5), (-300.0, 2000.0), (1e4, -1e4), (333.3, 777.7))
PROMPT_CASES = [(0, True), (1, False), (1, True), (2, False), (2, True), (10, False), (10, True)]         # (Np, boxes)
PROMPT_P = 9
MASK_KINDS = ("randn4", "zeros", "const7", "steps32", "randn1e4", "randn1e-4", "distinct")


def shared_p(G):
    return (1, G - 1, G, G + 1, 2 * G + 1)


RATIOS = {}


def _record(where, name, ratio):
    RATIOS[(where, name)] = max(RATIOS.get((where, name), 0.0), float(ratio))


def format_ratios(where):
    return "\n".join(f"  {n:<28s} {r:.3f}" for (w, n), r in sorted(RATIOS.items()) if w == where)


def check_bound(where, name, what, got, ref, bound):
    """[] or one failure ("bound", name, message, ratio); records the largest err / bound."""
    got = torch.as_tensor(got).double().cpu()
    ref, bound = ref.double().cpu(), bound.double().cpu()
    if not bool(torch.isfinite(got).all()):
        return [("bound", name, f"{what}: {name}: {int((~torch.isfinite(got)).sum())} elements are not finite (not written?)", math.inf)]
    ratio = float(((got - ref).abs() / bound).max())
    _record(where, name, ratio)
    if ratio > 1.0:
        i = int(((got - ref).abs() / bound).argmax())
        return [("bound", name, f"{what}: {name}: err / bound = {ratio:.3g} at flat index {i} (got {float(got.reshape(-1)[i])!r}, "
                                f"reference {float(ref.reshape(-1)[i])!r}, bound {float(bound.reshape(-1)[i]):.3g})", ratio)]
    return []


def check_exact(name, what, got, want):
    """[] or one failure ("exact", name, message, inf): the same bits."""
    g, w = _bits(got), _bits(want)
    if g.shape != w.shape or not np.array_equal(g, w):
        n = int((g != w).sum()) if g.shape == w.shape else -1
        i = int(np.flatnonzero(g.reshape(-1) != w.reshape(-1))[0]) if n > 0 else -1
        return [("exact", name, f"{what}: {name}: {n} elements differ in their bits (first at flat index {i})", math.inf)]
    return []


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().contiguous()
        return a.view(torch.int16 if a.element_size() == 2 else torch.int32).numpy()
    a = np.ascontiguousarray(a)
    return a.view(np.int16 if a.itemsize == 2 else np.int32)


# ------------------------------------------------------------------------------------------------------------------------------
# weights
# ------------------------------------------------------------------------------------------------------------------------------

def make_weights(seed=0, flat_ln2=False, small_c2=False):
    """Seeded prompt-encoder / mask_downscaling weights (numpy fp32).  The first convolution's bias is about 0.003, so that the variance the first
    LayerNorm2d sees on a flat mask (zeros, randn * 1e-4) is about 1e-5: there its epsilon is half of the normalisation.  ``flat_ln2``: the second LayerNorm2d's weight is
    about 0.02 and its bias about 1; ``small_c2``: see MASK_WEIGHT_SETS."""
    r = np.random.default_rng(seed)
    f = lambda *s, scale=1.0: (r.standard_normal(s) * scale).astype(np.float32)
    w = _weights(f)
    if flat_ln2:
        w["ln2_w"], w["ln2_b"] = f(16, scale=0.02), f(16)
    if small_c2:
        w["c2_w"], w["c2_b"] = f(16, 4, 2, 2, scale=0.001), f(16, scale=0.003)
    return w


def mask_weights(tag, seed=0):
    return make_weights(seed, flat_ln2=tag == "flat", small_c2=tag == "small2")


# The worst-case bound grows by the l1 norms of two 16-tap convolutions and by 2 / sig at each LayerNorm2d - about 200 times the 1.5e-6 that
# a rounding error, which accumulates like a random walk, reaches (measured on the host) - while the difference of the two GELU forms,
# 1e-4 .. 5e-4 per activation, passes the same stages without growing: on dense weights the forms are 1 - 7 bounds apart, not 10.  What
# enters the SECOND GELU's argument from upstream is scaled by |ln2_w|: with the "flat" set the bound in front of that GELU shrinks fifty
# times and its own two forms stand > 10 bounds apart in the output.  Both sets run every mask in both forms; the flag is asserted on "flat".
# "small2": the second convolution and its bias are about 0.001 / 0.003, so that the SECOND LayerNorm2d sees a variance of about 1e-5 too.
MASK_WEIGHT_SETS = ("dense", "flat", "small2")


def _weights(f):
    return {"pe_gauss": f(2, 128), "point_embed": f(4, 256), "not_a_point": f(256), "no_mask": f(256), "out_tokens": f(5, 256),
            "c1_w": f(4, 1, 2, 2, scale=0.5), "c1_b": f(4, scale=0.003), "ln1_w": 1 + f(4, scale=0.2), "ln1_b": f(4, scale=0.3),
            "c2_w": f(16, 4, 2, 2, scale=0.25), "c2_b": f(16, scale=0.1), "ln2_w": 1 + f(16, scale=0.2), "ln2_b": f(16, scale=0.3),
            "c3_w": f(256, 16, scale=0.25), "c3_b": f(256, scale=0.5)}


# ------------------------------------------------------------------------------------------------------------------------------
# Fourier features
# ------------------------------------------------------------------------------------------------------------------------------

def fourier(G, cx, cy, ex=None, ey=None):
    """float64 [..., 256] rows [sin | cos] and their bound for normalised coordinates cx, cy (float64 arrays of one shape); ex / ey: the
    error of x = 2 c - 1 the caller accounts for (default: the rounding of p + 0.5 and of the subtraction)."""
    G = G.astype(np.float64)
    two_pi = float(np.float32(2 * math.pi))
    x, y = (2 * cx - 1)[..., None], (2 * cy - 1)[..., None]
    ex = F32 * (np.abs(x + 1) + np.abs(x)) if ex is None else ex
    ey = F32 * (np.abs(y + 1) + np.abs(y)) if ey is None else ey
    a, b = x * G[0], y * G[1]
    v = two_pi * (a + b)
    dv = (two_pi * (np.abs(G[0]) * ex + np.abs(G[1]) * ey + F32 * (np.abs(a) + np.abs(b)) + F32 * np.abs(a + b)) + F32 * np.abs(v)) * SECOND
    s, c = np.sin(v), np.cos(v)
    return np.concatenate([s, c], -1), np.concatenate([dv + E_SINCOS * ULP * np.abs(s), dv + E_SINCOS * ULP * np.abs(c)], -1)


def sparse_count(Np, boxes):
    return Np + (2 if boxes else (1 if Np > 0 else 0))


def sparse_ref(w, points, labels, boxes):
    """PromptEncoder's sparse embeddings: (ref, bound, exact mask) float64 [P, Ns, 256]; rows are points -> padding (only without a
    box) -> the two box corners.  ``exact`` marks the rows that must equal not_a_point_embed bit for bit (ref holds it there)."""
    P = boxes.shape[0] if boxes is not None else points.shape[0]
    Np = 0 if points is None else points.shape[1]
    Ns = sparse_count(Np, boxes is not None)
    ref, bound, exact = np.zeros((P, Ns, C)), np.zeros((P, Ns, C)), np.zeros((P, Ns), bool)
    pe, nap = w["point_embed"].astype(np.float64), w["not_a_point"].astype(np.float64)
    if Np:
        c = (points.astype(np.float64) + 0.5) / 1024.0
        f, df = fourier(w["pe_gauss"], c[..., 0], c[..., 1])
        lab = labels[..., None]
        emb = np.where(lab == 0, pe[0], np.where(lab == 1, pe[1], 0.0))
        row = f + emb
        ref[:, :Np] = np.where(lab == -1, nap, row)
        bound[:, :Np] = np.where(lab == -1, 0.0, df + F32 * np.abs(row) * (emb != 0))
        exact[:, :Np] = labels == -1
    if Np and boxes is None:
        ref[:, Np], exact[:, Np] = nap, True
    if boxes is not None:
        c = (boxes.astype(np.float64).reshape(P, 2, 2) + 0.5) / 1024.0
        f, df = fourier(w["pe_gauss"], c[..., 0], c[..., 1])
        row = f + pe[2:4]
        ref[:, Ns - 2:], bound[:, Ns - 2:] = row, df + F32 * np.abs(row)
    return ref, bound + FLOOR, exact


def dense_pe_ref(w):
    """get_dense_pe(): float64 [4096, 256] and its bound; token t = 64 ty + tx at ((tx + 0.5) / 64, (ty + 0.5) / 64) - exact in fp32, so x
    carries the subtraction's rounding alone."""
    t = np.arange(T)
    cx, cy = ((t & 63) + 0.5) / 64.0, ((t >> 6) + 0.5) / 64.0
    ref, bound = fourier(w["pe_gauss"], cx, cy, ex=F32 * np.abs(2 * cx - 1)[:, None], ey=F32 * np.abs(2 * cy - 1)[:, None])
    return ref, bound + FLOOR


def prompt_inputs(Np, boxes, P=PROMPT_P):
    """points [P, Np, 2], labels [P, Np], boxes [P, 4] of the prompt-encoding table: every listed coordinate (x and y also from two
    different entries, so that the two rows of G are told apart), every label, boxes past the frame, the full frame, zero area."""
    pts = lab = bx = None
    if Np:
        pts, lab = np.zeros((P, Np, 2), np.float32), np.zeros((P, Np), np.int32)
        for p in range(P):
            for i in range(Np):
                k = p * Np + i
                pts[p, i] = (POINTS[k % 8][0], POINTS[(k // 8 + k) % 8][1]) if k >= 8 else POINTS[k]
                lab[p, i] = LABELS[(p + i) % 6]
    if boxes:
        kinds = [(-20.5, -10.0, 1100.0, 1050.25), (0.0, 0.0, 1023.0, 1023.0), (400.25, 300.5, 400.25, 300.5), (100.3, 50.7, 612.9, 999.1)]
        bx = np.array([kinds[p % 4] for p in range(P)], np.float32)
        bx[4:] += np.float32(3.0) * np.arange(P - 4, dtype=np.float32)[:, None]
    return pts, lab, bx


def check_prompt_rows(where, what, got, w, points, labels, boxes, name="sparse"):
    """The bound on every row, the exact rows bit for bit."""
    ref, bound, exact = sparse_ref(w, points, labels, boxes)
    fails = []
    if exact.any():
        fails += check_exact(name, what + " (label -1 / padding rows)", got[exact], np.broadcast_to(w["not_a_point"], got[exact].shape))
    if (~exact).any():
        fails += check_bound(where, name, what, got[~exact], torch.from_numpy(ref[~exact]), torch.from_numpy(bound[~exact]))
    return fails


# ------------------------------------------------------------------------------------------------------------------------------
# mask down-scaling
# ------------------------------------------------------------------------------------------------------------------------------

def gelu_exact(z):
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def _cubic(t):
    return ((CUBIC[0] * t + CUBIC[1]) * t + CUBIC[2]) * t + CUBIC[3]


def gelu_cubic(z):
    t = z.abs()
    return z.clamp(min=0.0) - t * torch.exp2(_cubic(t))


def _gelu_err(z, ez, exact):
    if exact:
        e = torch.erf(z / math.sqrt(2.0))
        own = 0.5 * z.abs() * (F32 + E_ERF * ULP * e.abs() + F32 * (1 + e.abs())) + 2 * F32 * gelu_exact(z).abs()
    else:
        t = z.abs()
        own = t * torch.exp2(_cubic(t)) * (math.log(2.0) * 3 * F32 * _cubic(t).abs() + E_EXP2 * ULP) + F32 * gelu_cubic(z).abs()
    return GELU_SLOPE * ez + own * SECOND


def _layernorm2d(a, ea, wt, bs):
    """LayerNorm2d over dim 1 of [P, n, h, w] in float64 and the bound of the docstring."""
    n = a.shape[1]
    wt, bs = wt.reshape(1, n, 1, 1), bs.reshape(1, n, 1, 1)
    mean = a.mean(1, keepdim=True)
    dev = a - mean
    sig = torch.sqrt((dev * dev).mean(1, keepdim=True) + LN_EPS)
    z = dev / sig * wt + bs
    E = ea + F32 * ((n - 1) * a.abs().mean(1, keepdim=True) + 2 * dev.abs())     # the mean's n - 1 adds, the centring
    Ebar, E2 = E.mean(1, keepdim=True), torch.sqrt((E * E).mean(1, keepdim=True))
    den = sig - E2
    assert bool((den > 0.5 * sig).all()), "the LayerNorm bound needs sig well above the input error"
    ez = wt.abs() * ((E + Ebar) / den + dev.abs() * E2 / (sig * den)) + (n + 8) * F32 * wt.abs() * dev.abs() / sig + F32 * z.abs()
    return z, ez * SECOND


def mask_ref(w, mask, exact):
    """PromptEncoder._embed_masks: (dense [P, 256, 64, 64], bound) in float64; ``mask`` fp32 [P, 256, 256]."""
    W = {k: torch.from_numpy(v).double().to(mask.device) for k, v in w.items()}
    conv = torch.nn.functional.conv2d
    x = mask.double()[:, None]
    a1 = conv(x, W["c1_w"], W["c1_b"], stride=2)
    e1 = 4 * F32 * conv(x.abs(), W["c1_w"].abs(), W["c1_b"].abs(), stride=2)
    z1, ez1 = _layernorm2d(a1, e1, W["ln1_w"], W["ln1_b"])
    g = gelu_exact if exact else gelu_cubic
    h1, eh1 = g(z1), _gelu_err(z1, ez1, exact)
    a2 = conv(h1, W["c2_w"], W["c2_b"], stride=2)
    e2 = conv(eh1, W["c2_w"].abs(), stride=2) + 17 * F32 * conv(h1.abs(), W["c2_w"].abs(), W["c2_b"].abs(), stride=2)
    z2, ez2 = _layernorm2d(a2, e2, W["ln2_w"], W["ln2_b"])
    h2, eh2 = g(z2), _gelu_err(z2, ez2, exact)
    w3 = W["c3_w"].reshape(256, 16, 1, 1)
    out = conv(h2, w3, W["c3_b"])
    bound = conv(eh2, w3.abs()) + 17 * F32 * conv(h2.abs(), w3.abs(), W["c3_b"].abs())
    return out, bound * SECOND + FLOOR


def keys_ref(w, emb, dense_ref, dense_bound, dtype):
    """The keys form of mask_src: (image embedding + dense prompt embedding) as the token-major stream [P, 4096, 256] and its bound."""
    e = emb.double().reshape(1, C, T)
    nm = torch.from_numpy(w["no_mask"]).double().to(emb.device).reshape(1, C, 1)
    c3b = torch.from_numpy(w["c3_b"]).double().to(emb.device).reshape(1, C, 1)
    d = dense_ref.reshape(-1, C, T)
    ref = e + d
    fp32 = F32 * ((e + nm).abs() + (c3b - nm).abs() + 2 * ref.abs()) + dense_bound.reshape(-1, C, T)
    bound = U16[dtype] * (ref.abs() + fp32) + SUB16[dtype] + fp32
    return ref.transpose(1, 2), bound.transpose(1, 2)


def make_masks(seed=1):
    """fp32 [7, 256, 256]: the mask inputs of the issue in the order of MASK_KINDS."""
    g = torch.Generator().manual_seed(seed)
    r = torch.randn(256, 256, generator=g)
    steps = torch.full((256, 256), -32.0)
    steps[40:171, 90:233] = 32.0                                       # _compute_logits_from_mask: +-32 with a blob inside
    yy, xx = torch.meshgrid(torch.arange(256.0), torch.arange(256.0), indexing="ij")
    distinct = 0.05 * (yy - 100.0) - 0.031 * (xx - 140.0) + 0.0004 * (yy - 7.0) * (xx - 31.0) / 16.0
    return torch.stack([r * 4, torch.zeros(256, 256), torch.full((256, 256), 7.0), steps, torch.randn(256, 256, generator=g) * 1e4,
                        torch.randn(256, 256, generator=g) * 1e-4, distinct]).float().contiguous()


# ------------------------------------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------------------------------------

def _softmax_bound(s, Sabs, V, n_s, exp_terms, dtype, round_probs, acc):
    """out = softmax(s) @ V and the bound of the docstring; s, Sabs [.., Nq, Nk], V [.., Nk, d]."""
    u, sub = U16[dtype], SUB16[dtype]
    smax = s.amax(-1, keepdim=True)
    R = smax - s.amin(-1, keepdim=True)
    Pm = torch.softmax(s, -1)
    out = Pm @ V
    eps = n_s * F32 * Sabs.amax(-1, keepdim=True) + F32 * (exp_terms[0] * R + exp_terms[1])
    g = torch.expm1(2 * eps)
    spread = torch.sqrt((Pm @ (V * V) - out * out).clamp(min=0.0))
    PV = Pm @ V.abs()
    b = g * spread + acc * F32 * (1 + g) * PV
    if round_probs:
        b = b + u * (1 + g) * PV
        if sub:
            b = b + sub * ((s - smax < math.log(2.0 ** -14) + 0.01).double() @ V.abs())
    return out, (b + u * (out.abs() + b) + sub) * SECOND + FLOOR


def self_attn_ref(q, k, v, P, Nt):
    """q, k, v 16-bit [P Nt, 256] -> (out, bound) float64 [P Nt, 256]."""
    hd = lambda x: x.double().reshape(P, Nt, H, 32).permute(0, 2, 1, 3)
    Q, K, V = hd(q), hd(k), hd(v)
    sc = 1.0 / math.sqrt(32.0)
    out, b = _softmax_bound(Q @ K.transpose(-1, -2) * sc, Q.abs() @ K.abs().transpose(-1, -2) * sc, V, 34, (3, 2), q.dtype, False, 64)
    back = lambda x: x.permute(0, 2, 1, 3).reshape(P * Nt, C)
    return back(out), back(b)


def t2i_ref(q, k, vT, P, Nt):
    """q 16-bit [P Nt, 128], k head-major [Pk, 8, 4096, 16], vT [Pk, 128, 4096] -> (out, bound) float64 [P Nt, 128]."""
    Q = q.double().reshape(P, Nt, H, 16).permute(0, 2, 1, 3)
    K = k.double()
    V = vT.double().reshape(-1, H, 16, T).transpose(-1, -2)
    out, b = _softmax_bound(Q @ K.transpose(-1, -2) / 4.0, Q.abs() @ K.abs().transpose(-1, -2) / 4.0, V, 32, (9, 70), q.dtype, True, 200)
    back = lambda x: x.permute(0, 2, 1, 3).reshape(P * Nt, CI)
    return back(out), back(b)


def _nonzero_ints(g, shape, hi):
    return (torch.randint(1, hi + 1, shape, generator=g) * (2 * torch.randint(0, 2, shape, generator=g) - 1)).float()


def make_self_case(family, P, Nt, dtype, seed=0):
    """dict(q, k, v [P Nt, 256] in ``dtype``; expect: None or the exact output)."""
    g = torch.Generator().manual_seed(1000 * seed + 16 * P + Nt)
    shape = (P, Nt, H, 32)
    expect = None
    if family == "uniform":
        q = torch.zeros(shape)
        k = torch.randint(-3, 4, shape, generator=g).float()
        m = torch.randint(-8, 9, (P, 1, H, 32), generator=g).float()
        d = torch.tensor([1.0] * (Nt - 1) + [-(Nt - 1.0)]).reshape(1, Nt, 1, 1)
        v = m + d * torch.randint(-2, 3, (P, 1, H, 32), generator=g).float()
        expect = m.expand(shape).clone()
    elif family == "onehot":
        assert dtype == torch.float16
        p_, i_, h_ = torch.meshgrid(torch.arange(P), torch.arange(Nt), torch.arange(H), indexing="ij")
        pi = (3 * i_ + p_ + 5 * h_) % Nt
        q, k = torch.zeros(shape), torch.zeros(shape)
        q.scatter_(3, ((pi + h_) % 32)[..., None], 16.0)
        k.scatter_(3, ((i_ + h_) % 32)[..., None], 16.0)
        v = _nonzero_ints(g, shape, 15)
        expect = torch.gather(v, 1, pi[..., None].expand(shape))
    else:
        q, k, v = (torch.randn(shape, generator=g) for _ in range(3))
        if family == "peaked":
            k = k * 6.0
    c = {n: x.reshape(P * Nt, C).to(dtype).contiguous() for n, x in (("q", q), ("k", k), ("v", v))}
    c["expect"] = None if expect is None else expect.reshape(P * Nt, C).to(dtype)
    return c


_DIGITS = torch.tensor([[(j >> (3 * i)) & 7 for i in range(4)] for j in range(T)]).float() * 2.0       # a_j in {0, 2, .., 14}^4
_LATTICE_DIMS, _NORM_DIM = [1, 6, 9, 14], 11


def onehot_target(P, Nt, variant):
    """pi [P, 8, Nt]: distinct for every (prompt, head, token) (variant 0) or on the edges of the 32-key steps and key quarters (1)."""
    p_, h_, t_ = torch.meshgrid(torch.arange(P), torch.arange(H), torch.arange(Nt), indexing="ij")
    if variant == 0:
        return (97 + 1031 * ((p_ * H + h_) * Nt + t_)) % T
    return torch.tensor(EDGE_KEYS)[(p_ + 5 * h_ + t_) % len(EDGE_KEYS)]


def make_t2i_case(family, P, Nt, kv_shared, dtype, seed=0):
    """dict(q [P Nt, 128], k [Pk, 8, 4096, 16], vT [Pk, 128, 4096] in ``dtype``; expect: None or the exact output [P Nt, 128])."""
    Pk = 1 if kv_shared else P
    g = torch.Generator().manual_seed(1000 * seed + 64 * P + 2 * Nt + kv_shared)
    expect = None
    fam, _, var = family.partition(":")
    if fam == "uniform":
        q = torch.zeros(P, H, Nt, 16)
        k = torch.randint(-3, 4, (Pk, H, T, 16), generator=g).float()
        v = torch.randint(-7, 8, (Pk, H, T, 16), generator=g).float()
        expect = (v.double().sum(2, keepdim=True) / T).float().expand(Pk, H, Nt, 16).expand(P, H, Nt, 16)
    elif fam == "onehot":
        assert dtype == torch.float16
        pi = onehot_target(P, Nt, int(var))                                                   # [P, 8, Nt]
        # prompt pk stores lattice point (j (2 pk + 1) + pk) mod 4096 at key j
        perm = torch.stack([(torch.arange(T) * (2 * pk + 1) + pk) % T for pk in range(Pk)])   # [Pk, T]
        a = _DIGITS[perm]                                                                      # [Pk, T, 4]
        k = torch.zeros(Pk, H, T, 16)
        k[..., _LATTICE_DIMS] = a[:, None]
        k[..., _NORM_DIM] = -(a * a).sum(-1)[:, None] / 2.0
        pk_of = torch.zeros(P, dtype=torch.long) if kv_shared else torch.arange(P)
        a_pi = a[pk_of[:, None, None], pi]                                                     # [P, 8, Nt, 4]
        q = torch.zeros(P, H, Nt, 16)
        q[..., _LATTICE_DIMS] = 64.0 * a_pi
        q[..., _NORM_DIM] = 64.0
        v = _nonzero_ints(g, (Pk, H, T, 16), 15)
        expect = v[pk_of[:, None, None], torch.arange(H)[None, :, None], pi]                  # [P, 8, Nt, 16]
    else:
        q = torch.randn(P, H, Nt, 16, generator=g)
        k = torch.randn(Pk, H, T, 16, generator=g)
        v = torch.randn(Pk, H, T, 16, generator=g)
        if fam != "diffuse":
            ramp = {"first": torch.linspace(20.0, -20.0, T), "rising": torch.linspace(-20.0, 20.0, T)}.get(fam)
            if ramp is None:                                                                   # needle: one key of the last 32
                ramp = torch.zeros(T)
                ramp[T - 6] = 15.0
            k[..., 0] = ramp
            q[..., 0] = 8.0
            k[..., 1:] *= 0.5
    c = {"q": q.permute(0, 2, 1, 3).reshape(P * Nt, CI).to(dtype).contiguous(), "k": k.to(dtype).contiguous(),
         "vT": v.permute(0, 1, 3, 2).reshape(Pk, CI, T).to(dtype).contiguous()}
    c["expect"] = None if expect is None else expect.permute(0, 2, 1, 3).reshape(P * Nt, CI).to(dtype)
    return c


def check_attention(where, name, what, got, case, ref_fn):
    """The exact expectation where the family has one, and the bound in every family."""
    fails = []
    if case["expect"] is not None:
        fails += check_exact(name, what, got, case["expect"])
    ref, bound = ref_fn()
    return fails + check_bound(where, name, what, got, ref, bound)


# ------------------------------------------------------------------------------------------------------------------------------
# source stream
# ------------------------------------------------------------------------------------------------------------------------------

def round16(x32, dtype):
    """fp32 numpy -> the 16-bit type (round to nearest even), as a torch tensor."""
    return torch.from_numpy(np.ascontiguousarray(x32, dtype=np.float32)).to(dtype)


def rounding_edge_values(n, seed=3):
    """fp32 [n]: random values with, in front, the cases a 16-bit rounding gets wrong: ties, fp16's subnormal range and its underflow,
    the overflow threshold, signed zeros."""
    r = np.random.default_rng(seed)
    x = (r.standard_normal(n) * np.exp(r.uniform(-12, 8, n))).astype(np.float32)
    edge = np.array([0.0, -0.0, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -20, 2.0 ** -14, 2.0 ** -15 + 2.0 ** -26, 2.0 ** -24,
                     2.0 ** -25, 2.0 ** -25 + 2.0 ** -40, 2.0 ** -26, 65504.0, 65519.0, 65520.0, -65520.0, 1e9, 3.0e-39, 2.0 ** -126], np.float32)
    x[:min(n, edge.size)] = edge[:n]
    return x


ADD_CAST_SIZES = (4, 1028, 8192 * 1024 + 1028)        # one vector; a partial last workgroup; past the 8192-workgroup cap (the grid-stride loop)


# ------------------------------------------------------------------------------------------------------------------------------
# the call layer: the raw C ABI on guarded buffers.  A subclass provides the memory (numpy on the host, torch on the device)
# ------------------------------------------------------------------------------------------------------------------------------

class Backend:
    """``lib`` with the prototypes of micro_sam_amd._lib._PROTOS set.  Subclasses: ``_in(np array) -> handle``, ``_out(nbytes) -> handle``
    (guard zones of PATTERN16 on both sides, the payload pre-filled with it), ``_ptr(handle)``, ``_read(handle, np dtype, shape)``,
    ``_guards_ok(handle)``, ``stream``, ``dtype`` (torch 16-bit type of the library), ``where``."""
    stream = None

    def _np16(self):
        return np.float16 if self.dtype == torch.float16 else np.uint16

    def _t16(self, h, shape):
        a = self._read(h, np.int16, shape)
        return torch.from_numpy(a).view(self.dtype)

    def _in16(self, t):
        return self._in(t.contiguous().view(torch.int16).numpy())

    def _call(self, fn, *args):
        status = getattr(self.lib, fn)(*args)
        assert status == 0, (fn, status, self.last_error())
        return status

    def _done(self, fn, outs):
        self.sync()
        for h in outs:
            assert self._guards_ok(h), f"{fn}: a guard zone was written"

    def sync(self):
        pass

    def params(self, w, exact_gelu=0):
        """(DecoderParams, MaskPromptParams, keep-alive list).  Every pointer the prompt-only head of a decode and
        msam_decoder_prepare_const read is set: the prompt encoder's from ``w``, the transformer's to shared seeded buffers."""
        from micro_sam_amd import _lib
        keep = []
        r = np.random.default_rng(11)
        w16 = self._in16((torch.from_numpy(r.standard_normal(2048 * 256).astype(np.float32)) / 16).to(self.dtype))
        b32 = self._in((r.standard_normal(4096) * 0.1).astype(np.float32))
        g32 = self._in((1 + r.standard_normal(4096) * 0.1).astype(np.float32))
        keep += [w16, b32, g32]
        dec = _lib.DecoderParams()

        def attn(a):
            for n in ("q", "k", "v", "o"):
                setattr(a, n + "_w", self._ptr(w16))
                setattr(a, n + "_b", self._ptr(b32))
        for L in dec.layer:
            attn(L.self_attn), attn(L.t2i), attn(L.i2t)
            for n in ("n1", "n2", "n3", "n4"):
                setattr(L, n + "_w", self._ptr(g32))
                setattr(L, n + "_b", self._ptr(b32))
            L.mlp1_w, L.mlp2_w, L.mlp1_b, L.mlp2_b = self._ptr(w16), self._ptr(w16), self._ptr(b32), self._ptr(b32)
        attn(dec.final_attn)
        dec.nf_w, dec.nf_b = self._ptr(g32), self._ptr(b32)
        for n in ("pe_gauss", "point_embed", "not_a_point", "no_mask", "out_tokens"):
            h = self._in(w[n])
            keep.append(h)
            setattr(dec, n, self._ptr(h))
        mp = _lib.MaskPromptParams()
        for n in ("c1_w", "c1_b", "ln1_w", "ln1_b", "c2_w", "c2_b", "ln2_w", "ln2_b", "c3_w", "c3_b"):
            h = self._in(w[n])
            keep.append(h)
            setattr(mp, n, self._ptr(h))
        mp.exact_gelu = exact_gelu
        return dec, mp, keep

    # ---- prompt encoding
    def prompt_encode(self, w, points, labels, boxes, mask=None, exact_gelu=0):
        """msam_prompt_encode -> (sparse fp32 [P, Ns, 256] or None, dense fp32 [P, 256, 64, 64] or None)."""
        dec, mp, keep = self.params(w, exact_gelu)
        P = next(x.shape[0] for x in (points, boxes, mask) if x is not None)
        Np = 0 if points is None else points.shape[1]
        Ns = sparse_count(Np, boxes is not None)
        hp, hl, hb, hm = (None if x is None else self._in(np.ascontiguousarray(x)) for x in (points, labels, boxes, mask))
        so = self._out(P * Ns * C * 4) if Ns else None
        do = self._out(P * C * T * 4) if mask is not None else None
        opt = lambda h: None if h is None else self._ptr(h)
        self._call("msam_prompt_encode", ctypes.byref(dec), ctypes.byref(mp), opt(hp), opt(hl), Np, opt(hb), opt(hm), P, opt(so), opt(do), self.stream)
        self._done("msam_prompt_encode", [h for h in (so, do) if h is not None])
        return (self._read(so, np.float32, (P, Ns, C)) if Ns else None, self._read(do, np.float32, (P, C, 64, 64)) if do is not None else None)

    def prompt_tokens(self, w, points, labels, boxes, refusal=False):
        """msam_decoder_prompt_prefix -> the block's first part: the tokens fp32 [P, Nt, 256] (prompt_tokens_kernel)."""
        dec, _, keep = self.params(w)
        P = next(x.shape[0] for x in (points, boxes) if x is not None)
        Np = 0 if points is None else points.shape[1]
        Nt = 5 + sparse_count(Np, boxes is not None)
        hp, hl, hb = (None if x is None else self._in(np.ascontiguousarray(x)) for x in (points, labels, boxes))
        nbytes = int(self.lib.msam_decoder_prompt_prefix_bytes(P, Nt))
        block = self._out(nbytes)
        wb = int(self.lib.msam_decoder_workspace_bytes(P))
        ws = self._scratch(wb)
        opt = lambda h: None if h is None else self._ptr(h)
        args = (ctypes.byref(dec), opt(hp), opt(hl), Np, opt(hb), P, self._ptr(block), self._ptr(ws), wb, self.stream)
        if refusal:
            status = self.lib.msam_decoder_prompt_prefix(*args)
            self.sync()
            return status == 1 and "at most 16 tokens" in self.last_error() and bool((self._read(block, np.int16, (nbytes // 2,)) == np.int16(PATTERN16)).all())
        self._call("msam_decoder_prompt_prefix", *args)
        self._done("msam_decoder_prompt_prefix", [block])
        return self._read(block, np.float32, (nbytes // 4,))[:P * Nt * C].reshape(P, Nt, C)

    def dense_pe(self, w):
        """msam_decoder_prepare_const -> the constants' first part: the dense positional encoding fp32 [4096, 256] (dense_pe_kernel)."""
        dec, _, keep = self.params(w)
        nbytes = int(self.lib.msam_decoder_const_bytes())
        consts = self._out(nbytes)
        self._call("msam_decoder_prepare_const", ctypes.byref(dec), self._ptr(consts), self.stream)
        self._done("msam_decoder_prepare_const", [consts])
        return self._read(consts, np.float32, (nbytes // 4,))[:T * C].reshape(T, C)

    # ---- attention
    def self_attention(self, c, P, Nt):
        hq, hk, hv = (self._in16(c[n]) for n in ("q", "k", "v"))
        out = self._out(P * Nt * C * 2)
        self._call("msam_dec_token_self_attention", self._ptr(hq), self._ptr(hk), self._ptr(hv), P, Nt, self._ptr(out), self.stream)
        self._done("msam_dec_token_self_attention", [out])
        return self._t16(out, (P * Nt, C))

    def upload_t2i(self, c):
        return tuple(self._in16(c[n]) for n in ("q", "k", "vT"))

    def t2i_attention(self, handles, kv_shared, group, P, Nt):
        hq, hk, hv = handles
        out = self._out(P * Nt * CI * 2)
        self._call("msam_dec_t2i_attention", self._ptr(hq), self._ptr(hk), self._ptr(hv), kv_shared, group, P, Nt, self._ptr(out), self.stream)
        self._done("msam_dec_t2i_attention", [out])
        return self._t16(out, (P * Nt, CI))

    # ---- source stream
    def source_stream(self, w, emb, mask=None, dense=None, P=1, exact_gelu=0):
        """msam_dec_source_stream -> (src_f32 [4096, 256] fp32, src16, keys16 [P, 4096, 256] or None)."""
        dec, mp, keep = self.params(w, exact_gelu)
        he = self._in(emb)
        hm, hd = (None if x is None else self._in(np.ascontiguousarray(x)) for x in (mask, dense))
        s32, s16 = self._out(T * C * 4), self._out(T * C * 2)
        k16 = self._out(P * T * C * 2) if (mask is not None or dense is not None) else None
        opt = lambda h: None if h is None else self._ptr(h)
        self._call("msam_dec_source_stream", ctypes.byref(dec), ctypes.byref(mp), self._ptr(he), opt(hm), opt(hd), P, self._ptr(s32), self._ptr(s16),
                   opt(k16), self.stream)
        self._done("msam_dec_source_stream", [h for h in (s32, s16, k16) if h is not None])
        return self._read(s32, np.float32, (T, C)), self._t16(s16, (T, C)), (None if k16 is None else self._t16(k16, (P, T, C)))

    def tokens_from_sparse(self, w, sparse, Ns, P):
        dec, _, keep = self.params(w)
        hs = None if sparse is None else self._in(sparse)
        n = P * (5 + Ns) * C
        outs = [self._out(n * 4), self._out(n * 4), self._out(n * 2)]
        self._call("msam_dec_tokens_from_sparse", ctypes.byref(dec), None if hs is None else self._ptr(hs), Ns, P, *[self._ptr(o) for o in outs], self.stream)
        self._done("msam_dec_tokens_from_sparse", outs)
        shape = (P, 5 + Ns, C)
        return self._read(outs[0], np.float32, shape), self._read(outs[1], np.float32, shape), self._t16(outs[2], shape)

    def add_cast(self, a, b, two):
        ha = self._in(a)
        hb = None if b is None else self._in(b)
        oa = self._out(a.size * 2)
        ob = self._out(a.size * 2) if two else None
        self._call("msam_dec_add_cast", self._ptr(ha), None if hb is None else self._ptr(hb), self._ptr(oa), None if ob is None else self._ptr(ob), a.size,
                   self.stream)
        self._done("msam_dec_add_cast", [o for o in (oa, ob) if o is not None])
        return self._t16(oa, (a.size,)), (None if ob is None else self._t16(ob, (a.size,)))


# ------------------------------------------------------------------------------------------------------------------------------
# the table, one function per group of kernels; each returns a list of failures (kind, output, message, ratio)
# ------------------------------------------------------------------------------------------------------------------------------

def run_sparse_case(be, w, Np, boxes, via="encode"):
    """sparse_embed_kernel (via="encode") or prompt_tokens_kernel (via="tokens") on one (Np, boxes) entry of the table: the bound on every row,
    not_a_point rows exactly, and the rows of labels outside {-1, 0, 1} as the bits of label 0 under a zeroed label-0 embedding."""
    pts, lab, bx = prompt_inputs(Np, boxes)
    what = f"Np={Np} boxes={boxes} via {via}"
    if via == "tokens" and 5 + sparse_count(Np, boxes) > 16:
        # 10 points and a box are 17 tokens: the prompt encoder takes them, a decode refuses them before any launch
        refused = be.prompt_tokens(w, pts, lab, bx, refusal=True)
        return [] if refused else [("exact", "prompt tokens", what + ": 17 tokens per prompt were not refused", math.inf)]
    name = "sparse rows" if via == "encode" else "prompt tokens"

    def rows(w_, lab_):
        if via == "encode":
            return be.prompt_encode(w_, pts, lab_, bx)[0]
        tok = be.prompt_tokens(w_, pts, lab_, bx)
        assert np.array_equal(_bits(tok[:, :5]), _bits(np.broadcast_to(w_["out_tokens"], tok[:, :5].shape))), f"{what}: the five output tokens are not copied exactly"
        return tok[:, 5:]
    got = rows(w, lab)
    fails = check_prompt_rows(be.where, what, got, w, pts, lab, bx, name)
    if Np and (lab > 1).any():
        w0 = dict(w, point_embed=w["point_embed"].copy())
        w0["point_embed"][0] = 0
        other = rows(w0, np.where(lab > 1, 0, lab).astype(np.int32))
        sel = lab > 1
        # (x + 0 turns a -0 into +0: a sine of -0, at the frame's centre, is -0 on its own and +0 after the zeroed embedding was added)
        fails += check_exact(name, what + " (labels outside {-1, 0, 1}: the pure Fourier row)", got[:, :Np][sel] + np.float32(0), other[:, :Np][sel] + np.float32(0))
    return fails


def run_dense_pe(be, w):
    ref, bound = dense_pe_ref(w)
    return check_bound(be.where, "dense pe", "dense_pe", be.dense_pe(w), torch.from_numpy(ref), torch.from_numpy(bound))


def run_masks(be, w, exact, emb=None, dev="cpu", tag="dense"):
    """mask_src_kernel's dense form on the seven masks (one launch, P = 7) and, with ``emb``, its keys form; ``tag`` names the weight set."""
    masks = make_masks()
    ref, bound = mask_ref(w, masks.to(dev), bool(exact))
    what = f"mask_src exact_gelu={exact} weights={tag}"
    name = f"mask dense {tag} " + ("erf" if exact else "cubic")
    got = be.prompt_encode(w, None, None, None, masks.numpy(), exact)[1]
    fails = []
    for i, kind in enumerate(MASK_KINDS):
        fails += check_bound(be.where, name, f"{what} {kind}", got[i], ref[i], bound[i])
    if emb is not None:
        kref, kbound = keys_ref(w, torch.from_numpy(emb).to(dev), ref, bound, be.dtype)
        s32, s16, keys = be.source_stream(w, emb, mask=masks.numpy(), P=len(MASK_KINDS), exact_gelu=exact)
        fails += check_bound(be.where, f"mask keys {tag} " + ("erf" if exact else "cubic"), what + " keys form", keys, kref, kbound)
    return fails, got, bound


def run_source_exact(be, w, P=3, seed=5):
    """src_prepare, dense_src: round16 of the fp32 sum bit for bit."""
    r = np.random.default_rng(seed)
    emb = (r.standard_normal((C, T)) * np.exp(r.uniform(-6, 3, (C, T)))).astype(np.float32)
    dense = r.standard_normal((P, C, T)).astype(np.float32)
    emb.reshape(-1)[:18] = rounding_edge_values(18)
    dense.reshape(P, -1)[:, :18] = 0
    s32, s16, keys = be.source_stream(w, emb, dense=dense, P=P)
    want32 = (emb + w["no_mask"][:, None]).T
    fails = check_exact("src_f32", "src_prepare", s32, want32)
    fails += check_exact("src16", "src_prepare", s16, round16(want32, be.dtype))
    fails += check_exact("dense keys", "dense_src", keys, round16((emb[None] + dense).transpose(0, 2, 1), be.dtype))
    s32b, s16b, none = be.source_stream(w, emb, P=1)
    assert none is None
    fails += check_exact("src_f32", "src_prepare alone", s32b, want32)
    return fails


def run_tokens_from_sparse(be, w):
    fails = []
    r = np.random.default_rng(7)
    for P, Ns in ((1, 0), (3, 1), (3, 11)):
        sparse = r.standard_normal((P, Ns, C)).astype(np.float32) if Ns else None
        want = np.concatenate([np.broadcast_to(w["out_tokens"], (P, 5, C))] + ([sparse] if Ns else []), 1)
        tok, qs, q16 = be.tokens_from_sparse(w, sparse, Ns, P)
        what = f"tokens_from_sparse P={P} Ns={Ns}"
        fails += check_exact("tokens", what, tok, want) + check_exact("queries", what, qs, want) + check_exact("queries16", what, q16, round16(want, be.dtype))
    return fails


def run_add_cast(be, sizes=ADD_CAST_SIZES):
    fails = []
    for n in sizes:
        a, b = rounding_edge_values(n, 3), rounding_edge_values(n, 4)[::-1].copy()
        b[:18] = 0
        if n >= 36:
            a[18:36], b[18:36] = rounding_edge_values(18), np.float32(2.0 ** -30)   # sums that round in fp32 before they round to 16 bit
        what = f"add_cast n={n}"
        fails += check_exact("add_cast", what + " (a + b)", be.add_cast(a, b, False)[0], round16(a + b, be.dtype))
        fails += check_exact("add_cast", what + " (b = NULL)", be.add_cast(a, None, False)[0], round16(a, be.dtype))
        oa, ob = be.add_cast(a, b, True)
        fails += check_exact("add_cast2 a", what, oa, round16(a + b, be.dtype)) + check_exact("add_cast2 b", what, ob, round16(a, be.dtype))
    return fails


def run_self_attention(be, P, Nt, families=SELF_FAMILIES, repeat=False, dev="cpu"):
    fails = []
    for fam in families:
        c = make_self_case(fam, P, Nt, be.dtype)
        what = f"self attention P={P} Nt={Nt} {fam}"
        got = be.self_attention(c, P, Nt)
        fails += check_attention(be.where, "self attention", what, got, c, lambda: self_attn_ref(c["q"].to(dev), c["k"].to(dev), c["v"].to(dev), P, Nt))
        if repeat:
            fails += check_exact("self attention", what + " (second call)", be.self_attention(c, P, Nt), got)
    return fails


def run_t2i(be, group, P, Nt, kv_shared, families=T2I_FAMILIES, repeat=False, neighbours=True, dev="cpu"):
    """One (kernel, P, Nt) entry: every family; for the shared kernel the first P - 1 prompts alone must give the same bits."""
    fails = []
    for fam in families:
        c = make_t2i_case(fam, P, Nt, kv_shared, be.dtype)
        what = f"t2i group={group} P={P} Nt={Nt} kv_shared={kv_shared} {fam}"
        name = f"t2i_shared<{group}>" if group else "t2i_attn"
        handles = be.upload_t2i(c)
        got = be.t2i_attention(handles, kv_shared, group, P, Nt)
        fails += check_attention(be.where, name, what, got, c, lambda: t2i_ref(c["q"].to(dev), c["k"].to(dev), c["vT"].to(dev), P, Nt))
        if repeat:
            fails += check_exact(name, what + " (second call)", be.t2i_attention(handles, kv_shared, group, P, Nt), got)
        if group and neighbours and P > 1:
            fewer = be.t2i_attention(handles, kv_shared, group, P - 1, Nt)
            fails += check_exact(name, what + " (the same prompts in a launch of P - 1)", fewer, got[:(P - 1) * Nt])
    return fails


def run_refusals(be, w):
    """Every new entry: return value 1, an error text, outputs untouched.  Returns the failures as strings."""
    bad = []
    z16 = be._in16(torch.zeros(2 * 16 * C, dtype=be.dtype))
    k16 = be._in16(torch.zeros(H * T * 16, dtype=be.dtype))
    f32 = be._in(np.zeros(T * C, np.float32))
    dec, mp, keep = be.params(w)
    D, M = ctypes.byref(dec), ctypes.byref(mp)
    p = be._ptr
    outs = [be._out(65536) for _ in range(3)]
    o = [p(h) for h in outs]
    calls = [
        ("msam_dec_token_self_attention", (p(z16), p(z16), p(z16), 1, 0, o[0], be.stream)),
        ("msam_dec_token_self_attention", (p(z16), p(z16), p(z16), 1, 17, o[0], be.stream)),
        ("msam_dec_token_self_attention", (p(z16), p(z16), p(z16), 0, 5, o[0], be.stream)),
        ("msam_dec_token_self_attention", (None, p(z16), p(z16), 1, 5, o[0], be.stream)),
        ("msam_dec_token_self_attention", (p(z16), p(z16), p(z16), 1, 5, None, be.stream)),
        ("msam_dec_t2i_attention", (p(z16), p(k16), p(k16), 1, 4, 1, 9, o[0], be.stream)),          # a group with more than 8 tokens
        ("msam_dec_t2i_attention", (p(z16), p(k16), p(k16), 0, 8, 1, 5, o[0], be.stream)),          # a group without the shared K / V
        ("msam_dec_t2i_attention", (p(z16), p(k16), p(k16), 1, 5, 1, 5, o[0], be.stream)),          # no such group
        ("msam_dec_t2i_attention", (p(z16), p(k16), p(k16), 1, 0, 1, 17, o[0], be.stream)),
        ("msam_dec_t2i_attention", (p(z16), p(k16), p(k16), 1, 0, -1, 9, o[0], be.stream)),
        ("msam_dec_t2i_attention", (p(z16), None, p(k16), 1, 0, 1, 9, o[0], be.stream)),
        ("msam_dec_source_stream", (D, M, p(f32), None, None, 0, o[0], o[1], o[2], be.stream)),
        ("msam_dec_source_stream", (D, M, None, None, None, 1, o[0], o[1], o[2], be.stream)),
        ("msam_dec_source_stream", (D, M, p(f32), p(f32), None, 1, o[0], o[1], None, be.stream)),   # a mask prompt without a keys output
        ("msam_dec_source_stream", (D, None, p(f32), p(f32), None, 1, o[0], o[1], o[2], be.stream)),
        ("msam_dec_source_stream", (D, M, p(f32), p(f32), p(f32), 1, o[0], o[1], o[2], be.stream)),
        ("msam_dec_tokens_from_sparse", (D, p(f32), 12, 1, o[0], o[1], o[2], be.stream)),
        ("msam_dec_tokens_from_sparse", (D, p(f32), -1, 1, o[0], o[1], o[2], be.stream)),
        ("msam_dec_tokens_from_sparse", (D, None, 2, 1, o[0], o[1], o[2], be.stream)),
        ("msam_dec_tokens_from_sparse", (D, p(f32), 2, 0, o[0], o[1], o[2], be.stream)),
        ("msam_dec_tokens_from_sparse", (D, p(f32), 2, 1, o[0], None, o[2], be.stream)),
        ("msam_dec_add_cast", (p(f32), p(f32), o[0], None, 6, be.stream)),
        ("msam_dec_add_cast", (p(f32), p(f32), o[0], None, 0, be.stream)),
        ("msam_dec_add_cast", (None, p(f32), o[0], None, 8, be.stream)),
        ("msam_dec_add_cast", (p(f32), None, o[0], o[1], 8, be.stream)),                            # the two-output form without b
        ("msam_dec_add_cast", (p(f32), p(f32), None, o[1], 8, be.stream)),
    ]
    for fn, args in calls:
        status = getattr(be.lib, fn)(*args)
        msg = be.last_error()
        if status != 1:
            bad.append(f"{fn}{args[3:-1]}: returned {status}, not 1")
        elif not msg.startswith(fn + ":"):
            bad.append(f"{fn}: error text {msg!r} does not name the entry")
    be.sync()
    for h in outs:
        if not (be._guards_ok(h) and bool((be._read(h, np.int16, (32768,)) == np.int16(PATTERN16)).all())):
            bad.append("a refused call wrote to an output")
    return bad


# ------------------------------------------------------------------------------------------------------------------------------
# the intrinsics on their own
# ------------------------------------------------------------------------------------------------------------------------------

def _ulps(got, ref64, allow=0.0):
    ulp = np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)
    return float((np.maximum(np.abs(got.astype(np.float64) - ref64) - allow, 0.0) / ulp).max())


def measure_intrinsics(be, w):
    """sinf / cosf: G1 = 0, G0 of 12 significant bits and points with x = k / 64 - 1 make x G0 exact, so the argument is the fp32 product
    fl(2 pi a) that numpy forms as well, and a label without an embedding leaves sin / cos themselves in the row.  erff and v_exp_f32: a
    zero second LayerNorm2d weight makes the second GELU's argument ln2_b exactly, a 0 / 1 third convolution copies the GELU out; erf
    form at z > 0 (allowing the roundings of 1 + erf and of the product), cubic form at z < 0 (g = -|z| 2^q with q from the kernel's
    three FMAs, redone in extended precision; allowing the product's rounding).  Returns the measured constants in ulp of the result."""
    r = np.random.default_rng(21)
    g0 = (r.integers(1, 4096, 128) * r.choice([-1, 1], 128)).astype(np.float64) * 2.0 ** r.integers(-28, -5, 128)
    wi = dict(w, pe_gauss=np.stack([g0, np.zeros(128)]).astype(np.float32))
    k = r.integers(0, 256, (9, 10))
    pts = np.stack([8.0 * k - 0.5, np.full(k.shape, 100.0)], -1).astype(np.float32)
    rows = be.prompt_encode(wi, pts, np.full(k.shape, 2, np.int32), None)[0][:, :10]
    a32 = ((k / 64.0 - 1.0)[..., None] * g0).astype(np.float32)
    assert np.array_equal(a32.astype(np.float64), (k / 64.0 - 1.0)[..., None] * g0)
    v = (np.float32(2 * math.pi) * a32).astype(np.float64)
    e_sin, e_cos = _ulps(rows[..., :128], np.sin(v)), _ulps(rows[..., 128:], np.cos(v))

    e_erf = e_exp2 = 0.0
    eye = np.zeros((256, 16), np.float32)
    eye[np.arange(256), np.arange(256) % 16] = 1
    zero_mask = np.zeros((1, 256, 256), np.float32)
    c = [np.longdouble(x) for x in CUBIC]
    f32 = lambda x: np.float32(x).astype(np.longdouble)
    for lo, hi in ((0.01, 0.2), (0.2, 1.0), (1.0, 2.5), (2.5, 4.0), (4.0, 6.0), (6.0, 9.0)):
        z = r.uniform(lo, hi, 16).astype(np.float32)
        wz = dict(w, ln2_w=np.zeros(16, np.float32), c3_w=eye, c3_b=np.zeros(256, np.float32))
        got = be.prompt_encode(dict(wz, ln2_b=z), None, None, None, zero_mask, 1)[1][0, :16, 0, 0]
        t = (z * np.float32(0.70710678118654752440)).astype(np.float64)
        e = np.array([math.erf(x) for x in t])
        g64 = 0.5 * z.astype(np.float64) * (1 + e)
        rounding = 0.5 * z * F32 * (1 + e) + F32 * g64
        ulp_e = np.spacing(e.astype(np.float32)).astype(np.float64)
        e_erf = max(e_erf, float((np.maximum(np.abs(got - g64) - rounding, 0.0) / (0.5 * z * ulp_e)).max()))
        got = be.prompt_encode(dict(wz, ln2_b=-z), None, None, None, zero_mask, 0)[1][0, :16, 0, 0]
        tl = z.astype(np.longdouble)
        q = f32(f32(f32(c[0] * tl + c[1]) * tl + c[2]) * tl + c[3])
        ex = np.exp2(q.astype(np.float64))
        ulp_x = np.spacing(ex.astype(np.float32)).astype(np.float64)
        g64 = -z.astype(np.float64) * ex
        e_exp2 = max(e_exp2, float((np.maximum(np.abs(got - g64) - F32 * np.abs(g64), 0.0) / (z * ulp_x)).max()))
    return {"sinf": e_sin, "cosf": e_cos, "erff": e_erf, "v_exp_f32": e_exp2}
