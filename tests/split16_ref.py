"""fp64 references, elementwise error bounds, seeded input generators and mutated references for the kernels of the split16 precision
mode (csrc/strict.hip): msam_strict_gemm (sgemm_kernel, split16 = 1 and - the same table - the fp32 product, split16 = 0),
msam_split16_prepare_pairs, msam_split16_t2i_attention (s16_t2i_fold_kernel, s16_t2i_kernel, s16_t2i_out_kernel) and the image -> token
block in both split16 forms, msam_split16_i2t_block (s16_i2t_fold_kernel, s16_i2t_kernel) and msam_strict_i2t_block with split16 = 1
(si2t_kernel<true>), msam_strict_upscale2 (s16_up2_kernel) and msam_split16_relpos_attention (srelpos_mfma_kernel<HD, true>,
srelpos_win_mfma_kernel<HD, true>).  A plain module: no fixtures, no kernel calls.  Everything is torch and follows the device of its operands; the
attention references work in chunks of prompts so that they also run on the device in fp64.

The references state the UNFUSED upstream formulation (torch.nn.functional.linear with the surrounding adds; Attention.forward of the
two-way transformer with its k / v projections; TwoWayAttentionBlock's image -> token step with norm4; output_upscaling[1:] and the
hyper product; the ViT block's attention with add_decomposed_rel_pos on zero-padded windows), so every fold is under test.

CONSTANTS, from the project's own statements (csrc/strict.hip header, strict.weight_scale), fixed before any measurement:
  F   = 2^-24  unit roundoff of fp32: one rounding of a value v costs F |v|
  H   = 2^-11  unit roundoff of fp16
  PAIR= 2^-22  an operand x enters the matrix pipe as hi = fp16(x), lo = fp16(x - hi); x - hi is exact in fp32 and |x - hi| <= H |x|, so
               |x - hi - lo| <= H^2 |x| = PAIR |x| while lo is a normal fp16 number
  SUB = 2^-25  below fp16's normal range (|lo| < 2^-14, i.e. |x| < 2^-3; or hi itself subnormal) the halves sit on the 2^-24 grid: the
               absolute error of the pair is <= SUB per SCALED element.  Activations enter unscaled (a_scale = 1): SUB per element;
               a weight is scaled by w_scale first: SUB / w_scale per element
               => pair(x, s) = PAIR |x| + SUB / s, and |lo| <= H |x| + SUB / s
  the dropped lo x lo term of a product: sum_k (H |a_k| + SUB)(H |w_k| + SUB / s) - PAIR sum |a||w| plus the floors
  fp16 x fp16 products are exact in fp32 (22 bits), so everything else is accumulation.
  MFMA model (the one tests/decoder_fold_ref.py states and the device has been held to): a v_mfma_f32_32x32x16_f16 step adds its 16
  products to the accumulator in an unspecified order; a product passes at most 16 roundings in its own step, the accumulator one per
  later step.  An f32-input v_mfma_f32_32x32x2_f32 step adds 2 products: 2 roundings.
  v_exp_f32: MI355X_MICROARCH.md makes no statement on its accuracy; 1 ulp (2 F relative) is the ISA guide's figure for the instruction,
  the one tests/decoder_kernels_ref.py (E_EXP2) already uses.  Its argument is formed by one fp32 subtraction: F |a| in the exponent.
  erff / expf (the product's GELU and sigmoid epilogues): the OpenCL full-profile table the device library is built to - erf 16 ulp,
  exp 3 ulp; IEEE division (2.5 ulp would be the table's figure: 5 F is used).
  Softmax: weights P_j = e^(s_j) / sum; a kernel whose scores (and exponentials, in the log domain) are off by at most eps computes
  P'_j = P_j e^(d_j) / sum_k P_k e^(d_k), |d| <= eps: |P'_j - P_j| <= (e^(2 eps) - 1) P_j, and because sum_j (P'_j - P_j) = 0,
  |sum_j P'_j X_j - U| <= (e^(2 eps) - 1) P @ |X - U| <= (e^(2 eps) - 1) sqrt(P @ X^2 - U^2) (Jensen).  No first-order step.

THE PRODUCT (``product_ref``).  out = act(((A + A2) W^T + b) cs + ct) + R with the 3 x 3 gather / the 2 x 2 scatter around it.  Per output:
  * x = a + a2 is one fp32 addition: F |x| (only where A2 is read).  e_a = pair(x, 1) (+ F |x|), e_w = pair(w, s).
  * the exact value of what the kernel sums, sum (a_hi + a_lo)(w_hi + w_lo) - a_lo w_lo, differs from sum x w by at most
        REP = e_a . |w| + (|x| + e_a) . e_w   and   LOLO = (H |x| + SUB) . (H |w| + SUB / s)
  * accumulation: nk = ceil(K / 32) k-tiles of 2 k-steps x 3 MFMAs, in the same k order in the 64 x 64, NBUF 1 and NBUF 2 kernels (so
    they give equal bits): a product passes <= 16 + (6 nk - 1) roundings: ACC = (6 nk + 15) F (1 + 2^-9) (|x| + e_a) . (|w| + e_w)
    (the three partial products of an element are at most (1 + 2^-10 + 2^-10) |x||w| together).  The scales are powers of two, exact.
    fp32 route (split16 = 0): no pair terms; 16 steps of 2 products per k-tile: ACC = (32 nk + 1) F |x| . |w|.
  * epilogue, value v with error e, step by step: + bias: e += 2 F (|v| + e) (product by out_scale exact, contraction or not);
    col_scale / col_shift: e = |cs| e + 2 F (|v cs| + |v cs + ct|); GELU 0.5 v (1 + erf(v / sqrt 2)): slope <= 1.13, own error
    0.5 |v| (F + 32 F |erf| + F (1 + |erf|)) + 2 F |gelu| (tests/decoder_kernels_ref.py); ReLU: slope 1, exact; sigmoid: slope 1/4,
    own 12 F sigma (expf 6 F of e^-v, the sum F, the division 5 F); + residual: e += F (|v + r| + e).
  Outside the domain (|x| a_scale or |w| w_scale >= 65504) a half is inf: the documented contract, asserted by the generators.

THE PREPARED PAIRS (``pairs_ref``): bit-exact, no bound.

THE t2i BOUND (``t2i_ref``).  T = 4096 keys, 8 heads x 16 channels, jh = (head, token slot).  xp = x + pos.
  * s16_t2i_fold_kernel: G[jh] = Wk_h^T q[j, h] / denom: 16 fmaf and one division, 17 F sum_c |q_c||Wk_c| / denom, then the pair of
    64 G: e_G = 17 F |q| . |Wk| / denom + pair(G, 64).  xp is one fp32 addition, then a pair: e_x = (F + PAIR) |xp| + SUB.
  * the score s = xp . G (256 products = 16 k-steps): REP and LOLO as above; two accumulators: hi x hi (16 MFMAs: 31 roundings of
    Sabs = (|xp| + e_x) . (|G| + e_G)) and the cross terms (32 MFMAs: 47 roundings at 2^-9 Sabs); their sum, the product with the
    rounded constant log2(e) / 64: 3 F |s|.     ds = REP + LOLO + (31 + 47 / 512) F Sabs + 3 F |s|
  * the exponentials, in the log domain: a key's weight passes its own v_exp_f32 (argument a, |a| <= 2 smax: F |a| + 2 F), and for each
    of the later tiles whose maximum grows the factor alpha = exp2(m_old - m_new) (2 F, its argument F |a|, the |a| telescope to
    <= 2 smax) and the product with it (F).  A tile t >= 1 CAN grow the kernel's maximum only if its true maximum exceeds the true
    running maximum of the tiles before it minus 2 max_j ds_j; g_t = 1 for these tiles, 0 otherwise, n_g = sum_t g_t <= 127:
        eps = max_j ds_j + F (4 smax + 2 + 3 n_g)
    perturbs the weights as stated under "Softmax".  The value projection is linear, so the perturbed weights reach the output as
    sum_j (P'_j - P_j)(V_j - out) with V = X Wv^T: (e^(2 eps) - 1) sqrt(P @ V^2 - (P @ V)^2) per OUTPUT channel - no triangle
    inequality over the 256 stream channels.  Everything below is an error of U = P'^T X per stream channel and passes |Wv|.
  * the exponentials enter the second product as pairs of 4096 p (p <= 1; l >= 1 after the last rescale because the largest key of a jh
    has p = 1), X as pairs: e^(2 eps) P @ (pair terms of X) + (PAIR P + SUB / 4096) @ |X| + LOLO.
  * accumulation of U, magnitude-aware: the accumulator after tile t holds (in units of the final l) A_t = sum over the keys of tiles
    <= t of P |X|.  A tile is 6 MFMAs on one accumulator plus its rescale: (6 + g_t) F A_t per tile, and 16 F of the tile's own products:
        ACC_U = F (sum_t (6 + g_t) A_t + 16 A_127)       (a needle in the last tile costs 22 F, a flat row ~ 470 F of P @ |X|)
  * l: a 16-term tree per tile (4 F), Kahan-compensated across the tiles (2 F), n_g rescales (F each), the final l - lc, the lane
    pair's sum and the IEEE division (3 F): (9 + n_g) F relative, on |U| <= P @ |X|; the product with 1 / l: F more.
  * s16_t2i_out_kernel: out = Wv_h U + bv, a 256-term fmaf chain and one addition: |Wv| . e_U + 257 F |Wv| . (|U| + e_U) + F |out|.

THE i2t BOUNDS (``i2t_ref(form=...)``), pre-norm row r = x + sum_h softmax_j(s[h, :]) (Wo_h v[j, h]) + bo with error E per channel:
  form "folded" (msam_split16_i2t_block):
  * G[h j] = Wq_h^T k[j, h] / denom and beta = bq_h . k[j, h] / denom (17 F, as above), pair of 64 G; xp as above.  The score: REP +
    LOLO + (31 + 47 / 512) F Sabs, then (sum) / 64 + beta and the product with log2(e): 4 F (|s| + |beta|) + e_beta; one exponential
    relative to the head's maximum: F (2 smax + 2).  eps[row, h] = max_j of the sum.
  * the NORMALISED probabilities 4096 p / l (l: 8 terms, 7 F; the division and the product: 3 F relative) enter as pairs; VO[h j] =
    Wo[:, h] v[j, h] (16 fmaf: 16 F |Wo| . |v|) as pairs of 64 VO.  With dev = sqrt(a @ VO^2 - (a @ VO)^2) per head:
        E = sum_h (e^(2 eps_h) - 1) dev_h + e^(2 eps) (10 F a @ |VO| + a @ e_VO + (PAIR a + SUB / 4096) @ (|VO| + e_VO) + LOLO)
  * accumulation: 4 k-steps x 3 MFMAs on one accumulator: (16 + 11) F a @ |VO|; x io + bo, + x: 3 F (|r| + |bo|).
  * LayerNorm, two-pass statistics in fp32, carried through without linearising exactly as tests/decoder_fold_ref.py derives it: with
    dmu = 260 F mean (|r| + E) (the 256-term sum of the lane pair), Ebar = mean E + dmu, E2 = rms E + dmu + 70 F sig (the deviations'
    rounding, their squares' 128-term fmaf chain and the exchange: 133 F relative on the variance, half of it on sig; sqrtf, the division),
        |y' - y| <= |w| ((E + Ebar) / (sig - E2) + |dev| E2 / (sig (sig - E2))) + 8 F (|r| + |mu|) |w| / (sig - E2) + 2 F |b| + F |y|
  form "unfolded" (si2t_kernel<true>, Tk <= 16): q = xp Wq^T (K = 256: 8 k-tiles, pairs of xp and of w_scale Wq) + bq, scores
    q . k on the vector unit (8 fmaf per lane half, the exchange, the product with the rounded log2(e) / denom: 11 F), softmax with
    v_exp_f32, l a 16-term sum, 1 / l and the product (17 F), P @ v (Tk fmaf), projection by Wo (K = 128: 4 k-tiles, pairs of the
    attention output and of w_scale Wo), + bo + x, LayerNorm as above.  The terms are assembled in ``_i2t_chunk``.

THE up2 AND relpos BOUNDS (``up2_ref``: msam_strict_upscale2; ``relpos_ref``: msam_split16_relpos_attention) are derived in the comment
blocks in front of these references, from the same constants.

Every generator asserts on the CPU that it stays inside the documented domain (|x + pos| < 2^15, |score| log2 e <= 30, folded operands
x 64 inside fp16's range).  *_MUTATIONS name the defects these kernels are prone to as arguments of the references;
tests/test_split16_ref_host.py proves each at least 4 bounds from the truth on some generator, which keeps the bounds from being slack."""
import math

import torch

F32 = 2.0 ** -24
H16 = 2.0 ** -11
PAIR = 2.0 ** -22
SUB = 2.0 ** -25
FP16_MAX = 65504.0
T, NH, HD, C, CI = 4096, 8, 16, 256, 128
LOG2E = 1.4426950408889634
ACT_NONE, ACT_GELU, ACT_RELU, ACT_SIGMOID = 0, 1, 2, 3
E_ERF_ULP = 16.0
GELU_SLOPE = 1.13

PRODUCT_MUTATIONS = ("drop_a_lo", "drop_w_lo", "drop_last_ktile", "scale_not_undone", "a2_on_all_cols", "res_not_wrapped",
                     "neighbour_bias", "no_act", "shuffle_kykx_swapped", "conv_no_pad", "conv_tap_shift")
T2I_MUTATIONS = ("drop_last_tile", "no_rescale", "pos_in_values", "pad_unmasked", "swap_heads", "prompt_from_next", "no_bv",
                 "drop_p_lo", "drop_x_lo", "drop_score_lo")
I2T_MUTATIONS = ("pad_unmasked", "no_beta", "no_bo", "no_residual", "swap_heads", "neighbour_tokens", "shared_read_per_prompt",
                 "drop_lo")
# (UP2_MUTATIONS: next to the up2 reference below)


def weight_scale(w):
    """strict.weight_scale without its cache: the power of two that brings max |w| into (2^12, 2^13]."""
    m = float(w.abs().max())
    sc = 1.0 if not (m > 0.0 and math.isfinite(m)) else 2.0 ** (13 - math.ceil(math.log2(m)))
    return min(max(sc, 2.0 ** -40), 2.0 ** 40)


def hi16(x):
    """fp64 value of fp16(x) for an fp32 / fp64 tensor of fp32 values."""
    return x.float().half().double()


def pair16(x):
    """fp64 value of hi + lo for fp32 values x (both halves rounded as the kernels round them)."""
    x = x.float()
    hi = x.half()
    lo = (x - hi.float()).half()
    return hi.double() + lo.double()


def _pair_err(xabs, scale=1.0):
    return PAIR * xabs + SUB / scale


def _lo_abs(xabs, scale=1.0):
    return H16 * xabs + SUB / scale


def to_device(inp, dev):
    return {n: (t.to(dev) if torch.is_tensor(t) else t) for n, t in inp.items()}


# --------------------------------------------------------------------------------------------------------------------- the product
def _gather3x3(x, no_pad=False, tap_shift=False):
    """x fp64 [B, h, w, c] -> [B h w, 9 c], columns (ky, kx, c), zero outside the image (padding = 1)."""
    B, h, w, c = x.shape
    flat = x.reshape(B * h * w, c)
    m = torch.arange(B * h * w, device=x.device)
    py, px = (m // w) % h, m % w
    cols = []
    for tap in range(9):
        t = (tap + 1) % 9 if tap_shift else tap
        dy, dx = t // 3 - 1, t % 3 - 1
        src = (m + dy * w + dx).clamp(0, B * h * w - 1)
        v = flat[src]
        if not no_pad:                                                                   # no_pad: the neighbour in memory instead of zero
            inside = (py + dy >= 0) & (py + dy < h) & (px + dx >= 0) & (px + dx < w)
            v = v * inside[:, None]
        cols.append(v)
    return torch.cat(cols, dim=1)


def _scatter2x2(y, B, h, w, c, swapped=False):
    """y [B h w, 4 c] columns (ky * 2 + kx) * c + co -> [B * 2h * 2w, c] rows (b, 2 y + ky, 2 x + kx)."""
    t = y.reshape(B, h, w, 2, 2, c)
    if swapped:
        t = t.transpose(3, 4)
    return t.permute(0, 1, 3, 2, 4, 5).reshape(B * 2 * h * 2 * w, c)


def _act(v, act):
    if act == ACT_GELU:
        return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))
    if act == ACT_RELU:
        return torch.relu(v)
    if act == ACT_SIGMOID:
        return torch.sigmoid(v)
    return v


def product_ref(inp, mutation=None, split=True):
    """``inp``: a dict of make_product -> (ref, bound), fp64 [M, N] ([4 M, N / 4] for the 2 x 2 store); with a mutation (ref, None)."""
    assert mutation is None or mutation in PRODUCT_MUTATIONS, mutation
    w = inp["w"].double()
    N, K = w.shape
    s = float(inp.get("w_scale") or 1.0)
    conv, shuf = inp.get("conv"), inp.get("shuffle")
    if conv:
        a = _gather3x3(inp["a"].double().reshape(*conv), mutation == "conv_no_pad", mutation == "conv_tap_shift")
    else:
        a = inp["a"].double()
    M = a.shape[0]
    rows = torch.arange(M, device=a.device)
    a2 = inp.get("a2")
    a2_cols = 0 if mutation == "a2_on_all_cols" else int(inp.get("a2_cols") or 0)
    x2 = None
    if a2 is not None:
        x2 = a + a2.double()[rows % (int(inp.get("a2_rows") or 0) or M)]

    def prod(x, wm):
        if mutation == "drop_a_lo":
            x = hi16(x)
        if mutation == "drop_w_lo":
            wm = hi16(wm * s) / s
        if mutation == "drop_last_ktile":
            x = x.clone()
            x[:, 32 * ((K - 1) // 32):] = 0.0
        return x @ wm.t()

    if x2 is None:
        y = prod(a, w)
    elif a2_cols:
        y = torch.cat([prod(x2, w[:a2_cols]), prod(a, w[a2_cols:])], dim=1)
    else:
        y = prod(x2, w)
    if mutation == "scale_not_undone":
        y = y * s
    bias = inp.get("bias")
    v = y
    if bias is not None:
        v = v + (torch.roll(bias.double(), -1) if mutation == "neighbour_bias" else bias.double())
    cs, ct = inp.get("col_scale"), inp.get("col_shift")
    if cs is not None:
        v = v * cs.double() + ct.double()
    act = int(inp.get("act") or 0)
    z = v
    if mutation != "no_act":
        v = _act(v, act)
    res = inp.get("res")
    if res is not None:
        rr = int(inp.get("res_rows") or 0) or M
        v = v + res.double()[rows.clamp(max=rr - 1) if mutation == "res_not_wrapped" else rows % rr]
    out = _scatter2x2(v, *shuf, swapped=mutation == "shuffle_kykx_swapped") if shuf else v
    if mutation is not None:
        return out, None
    # ---- the bound of the module docstring
    nk = (K + 31) // 32
    wa = w.abs()

    def perr(x, added):
        xa = x.abs()
        if not split:
            ea = F32 * xa if added else torch.zeros_like(xa)
            return ea @ wa.t() + (32 * nk + 1) * F32 * ((xa + ea) @ wa.t())
        ea = _pair_err(xa) + (F32 * xa if added else 0.0)
        ew = _pair_err(wa, s)
        rep = ea @ wa.t() + (xa + ea) @ ew.t()
        lolo = _lo_abs(xa) @ _lo_abs(wa, s).t()
        acc = (6 * nk + 15) * F32 * (1 + 2.0 ** -9) * ((xa + ea) @ (wa + ew).t())
        return rep + lolo + acc

    if x2 is None:
        e = perr(a, False)
    elif a2_cols:
        e = torch.cat([perr(x2, True)[:, :a2_cols], perr(a, False)[:, a2_cols:]], dim=1)
    else:
        e = perr(x2, True)
    v = y
    if bias is not None:
        v = y + bias.double()
    e = e + 2 * F32 * (v.abs() + e)
    if cs is not None:
        v2 = v * cs.double() + ct.double()
        e = cs.double().abs() * e + 2 * F32 * ((v * cs.double()).abs() + v2.abs())
        v = v2
    assert torch.equal(v, z)
    if act == ACT_GELU:
        erf = torch.erf(v / math.sqrt(2.0))
        own = 0.5 * v.abs() * (F32 + 2 * E_ERF_ULP * F32 * erf.abs() + F32 * (1 + erf.abs())) + 2 * F32 * _act(v, act).abs()
        e = GELU_SLOPE * e + own
    elif act == ACT_SIGMOID:
        e = 0.25 * e + 12 * F32 * torch.sigmoid(v)
    v = _act(v, act)
    if res is not None:
        v = v + res.double()[rows % (int(inp.get("res_rows") or 0) or M)]
        e = e + F32 * (v.abs() + e)
    return out, (_scatter2x2(e, *shuf) if shuf else e)


PRODUCT_GENERATORS = ("diffuse", "magnitudes", "distinct")


def make_product(name, M, N, K, seed=0, bias=False, act=ACT_NONE, a2_rows=None, a2_cols=0, res_rows=None, col_affine=False, shuffle=None,
                 conv=None, w_range=0):
    """Seeded operands of one msam_strict_gemm call, on the CPU (fp32).

    diffuse     a ~ randn, w ~ randn / sqrt(K)
    magnitudes  the rows of a scaled log-uniformly over 2^-12 .. 2^10: the bound's absolute (SUB) and relative terms trade places
    distinct    diffuse, plus a signature per row of a (+-1 pattern of the row index), per column of w, per bias / residual entry, so a
                crossed row, column or k index moves the result far
    a2_rows / res_rows: None = absent, 0 = one row per output row, n = n rows wrapped; shuffle = (B, h, w, c) with M = B h w, N = 4 c;
    conv = (B, h, w, c) with M = B h w, K = 9 c; w_range = r: the columns of w scaled over 2^-r .. 1 (w_scale follows the largest)."""
    assert name in PRODUCT_GENERATORS, name
    g = torch.Generator().manual_seed(100003 * seed + 97 * M + 31 * N + K + 7 * PRODUCT_GENERATORS.index(name))

    def rn(*shape):
        return torch.randn(*shape, generator=g)

    if conv:
        assert M == conv[0] * conv[1] * conv[2] and K == 9 * conv[3], (M, K, conv)
        a = rn(M, conv[3])
    else:
        a = rn(M, K)
    w = rn(N, K) / math.sqrt(K)
    if name == "magnitudes":
        a = a * torch.exp2(torch.rand(M, 1, generator=g) * 22 - 12)
    if name == "distinct":
        a = a + 0.5 * (1.0 - 2.0 * ((torch.arange(M)[:, None] >> (torch.arange(a.shape[1])[None, :] % 8)) & 1).float())
        w = w + (0.5 / math.sqrt(K)) * (1.0 - 2.0 * ((torch.arange(N)[:, None] >> (torch.arange(K)[None, :] % 8)) & 1).float())
    if w_range:
        w = w * torch.exp2(-torch.rand(N, 1, generator=g) * w_range)
        w[0] = w[0] / w[0].abs().max()                                                    # one row keeps the largest weight at 1
    inp = {"a": a.contiguous(), "w": w.contiguous(), "act": act, "a2_cols": a2_cols, "shuffle": shuffle, "conv": conv}
    if bias:
        inp["bias"] = rn(N) + (torch.arange(N).float() % 5 if name == "distinct" else 0.0)
    if a2_rows is not None:
        inp["a2"], inp["a2_rows"] = rn(a2_rows or M, K), a2_rows
    if res_rows is not None:
        inp["res"], inp["res_rows"] = rn(res_rows or M, N) + torch.arange(res_rows or M).float()[:, None] % 7, res_rows
    if col_affine:
        inp["col_scale"], inp["col_shift"] = rn(N) * 0.3 + 1.0, rn(N)
    inp["w_scale"] = weight_scale(inp["w"])
    check_product_domain(inp)
    return inp


def check_product_domain(inp):
    x = inp["a"].abs().max().item() + (inp["a2"].abs().max().item() if inp.get("a2") is not None else 0.0)
    assert x < FP16_MAX and inp["w"].abs().max().item() * inp["w_scale"] < FP16_MAX, "operands outside fp16's range"
    assert 2.0 ** 12 < inp["w"].abs().max().item() * inp["w_scale"] <= 2.0 ** 13


# (M, N, K, options of make_product): the axis of the device test, one table for the three tile routes and for split16 = 0.  M, N, K are
# paired over M in {1, 63, 64, 65, 127, 128, 129, 200}, N in {4, 60, 64, 65, 128, 132}, K in {4, 28, 32, 36, 64, 260}.
PRODUCT_CASES = [
    ("diffuse", 1, 4, 4, {}),
    ("diffuse", 63, 60, 28, {"bias": True}),
    ("diffuse", 64, 64, 32, {"bias": True, "act": ACT_GELU}),
    ("diffuse", 65, 65, 36, {"bias": True, "act": ACT_RELU}),
    ("diffuse", 127, 128, 64, {"bias": True, "act": ACT_SIGMOID}),
    ("diffuse", 128, 132, 260, {"bias": True}),
    ("diffuse", 129, 4, 260, {}),
    ("diffuse", 200, 60, 4, {"bias": True, "act": ACT_GELU}),
    ("magnitudes", 200, 132, 36, {"bias": True}),
    ("magnitudes", 65, 64, 260, {}),
    ("distinct", 129, 65, 64, {"bias": True, "res_rows": 0}),
    ("distinct", 200, 128, 28, {"bias": True, "a2_rows": 7, "res_rows": 11, "act": ACT_GELU}),
    ("distinct", 128, 60, 32, {"a2_rows": 0}),
    ("distinct", 200, 256, 36, {"bias": True, "a2_rows": 50, "a2_cols": 128}),
    ("distinct", 127, 132, 64, {"bias": True, "col_affine": True, "act": ACT_RELU}),
    ("diffuse", 63, 65, 260, {"w_range": 20}),
    ("distinct", 70, 64, 36, {"bias": True, "col_affine": True, "act": ACT_GELU, "shuffle": (2, 5, 7, 16)}),
    ("distinct", 70, 132, 28, {"bias": True, "shuffle": (2, 5, 7, 33)}),
    ("distinct", 70, 65, 72, {"bias": True, "conv": (2, 5, 7, 8), "act": ACT_RELU}),
    ("distinct", 70, 4, 72, {"conv": (2, 5, 7, 8), "res_rows": 35}),
]


def product_case_id(case):
    name, M, N, K, opt = case
    return f"{name}-{M}x{N}x{K}" + "".join(f"-{k}{'' if v is True else v}" for k, v in opt.items()).replace(" ", "")


# the case on which each mutation is shown (tests/test_split16_ref_host.py)
PRODUCT_MUTATION_CASE = {
    "drop_a_lo": ("diffuse", 65, 65, 36, {}), "drop_w_lo": ("diffuse", 65, 65, 36, {}),
    "drop_last_ktile": ("diffuse", 65, 65, 36, {}), "scale_not_undone": ("diffuse", 65, 65, 36, {}),
    "a2_on_all_cols": PRODUCT_CASES[13], "res_not_wrapped": PRODUCT_CASES[11], "neighbour_bias": PRODUCT_CASES[10],
    "no_act": PRODUCT_CASES[11], "shuffle_kykx_swapped": PRODUCT_CASES[17], "conv_no_pad": PRODUCT_CASES[18],
    "conv_tap_shift": PRODUCT_CASES[18],
}


# ------------------------------------------------------------------------------------------------------------------ prepared pairs
def pairs_ref(w, scale, permute):
    """msam_split16_prepare_pairs, bit for bit: w fp32 [N, K] (K % 32 == 0) -> fp16 [N, 2 K]: per row K / 32 k-tiles of [32 hi | 32 lo];
    permute: channels 4 j .. 4 j + 3 of a k-tile sit at (j >> 2) * 16 + (j & 1) * 8 + ((j >> 1) & 1) * 4."""
    N, K = w.shape
    x = w.float() * scale
    hi = x.half()
    lo = (x - hi.float()).half()
    j = torch.arange(8, device=w.device)
    pos = ((j >> 2) * 16 + (j & 1) * 8 + ((j >> 1) & 1) * 4) if permute else j * 4
    idx = (pos[:, None] + torch.arange(4, device=w.device)[None, :]).reshape(32)          # source channel c of a k-tile -> slot
    out = torch.empty(N, K // 32, 2, 32, dtype=torch.float16, device=w.device)
    out[:, :, 0, idx] = hi.reshape(N, K // 32, 32)
    out[:, :, 1, idx] = lo.reshape(N, K // 32, 32)
    return out.reshape(N, 2 * K)


# ----------------------------------------------------------------------------------------------------------------------------- t2i
def _heads(t):
    """[..., 128] -> [..., 8, 16]"""
    return t.reshape(*t.shape[:-1], NH, HD)


def _t2i_chunk(inp, lo, hi, mutation):
    B, Tk = inp["q"].shape[:2]
    n = hi - lo
    denom = float(inp["denom"])
    X = inp["keys"][lo:hi].double()                                                       # [n, T, 256]
    pos = inp["pos"].double()
    if mutation == "pad_unmasked":                                                        # the 8 slots counted as tokens: row 8 p + j
        rows = (torch.arange(lo, hi)[:, None] * 8 + torch.arange(Tk)[None, :]) % (B * Tk)
        q = inp["q"].double().reshape(B * Tk, CI)[rows.to(X.device)]
    else:
        q = inp["q"][lo:hi].double()
    q = _heads(q).permute(0, 2, 1, 3)                                                     # [n, 8, Tk, 16]
    wk, wv = inp["wk"].double().reshape(NH, HD, C), inp["wv"].double().reshape(NH, HD, C)
    bv = inp["bv"].double().reshape(NH, 1, HD)
    xp = X + pos
    if mutation == "drop_x_lo":
        X, xp = hi16(X), hi16(xp)
    G = torch.einsum("nhtd,hdc->nhtc", q, wk) / denom                                     # [n, 8, Tk, 256]
    s = torch.einsum("njc,nhtc->nhtj", xp, G)                                             # [n, 8, Tk, T]
    if mutation == "drop_score_lo":                                                       # the score product without its two cross terms
        s = torch.einsum("njc,nhtc->nhtj", hi16(xp), hi16(64.0 * G) / 64.0)
    sm = s
    if mutation == "drop_last_tile":
        sm = s.clone()
        sm[..., T - 32:] = -math.inf
    P = torch.softmax(sm, dim=-1)
    Xv = xp if mutation == "pos_in_values" else X
    if mutation == "no_rescale":                                                          # U keeps the maximum of the tile it was added in
        mrun = torch.cummax(s.reshape(*s.shape[:-1], 128, 32).amax(dim=-1), dim=-1)[0]    # [n, 8, Tk, 128]
        pu = torch.exp(s - mrun.repeat_interleave(32, dim=-1))
        U = torch.einsum("nhtj,njc->nhtc", pu, Xv) / torch.exp(s - s.amax(dim=-1, keepdim=True)).sum(dim=-1, keepdim=True)
    elif mutation == "drop_p_lo":
        p = torch.exp(s - s.amax(dim=-1, keepdim=True))
        U = torch.einsum("nhtj,njc->nhtc", hi16(p * 4096.0) / 4096.0, Xv) / p.sum(dim=-1, keepdim=True)
    else:
        U = torch.einsum("nhtj,njc->nhtc", P, Xv)                                         # [n, 8, Tk, 256]
    out = torch.einsum("nhtc,hdc->nhtd", U, wv) + (0.0 if mutation == "no_bv" else bv)
    if mutation is not None:
        return out, None
    # ---- the bound of the module docstring
    qa, wka, wva, Xa, xpa, Ga = q.abs(), wk.abs(), wv.abs(), X.abs(), xp.abs(), G.abs()
    eG = 17 * F32 * torch.einsum("nhtd,hdc->nhtc", qa, wka) / denom + _pair_err(Ga, 64.0)
    ex = (F32 + PAIR) * xpa + SUB
    rep = torch.einsum("njc,nhtc->nhtj", ex, Ga) + torch.einsum("njc,nhtc->nhtj", xpa + ex, eG)
    lolo = torch.einsum("njc,nhtc->nhtj", _lo_abs(xpa), _lo_abs(Ga, 64.0))
    sabs = torch.einsum("njc,nhtc->nhtj", xpa + ex, Ga + eG)
    ds = rep + lolo + (31 + 47.0 / 512) * F32 * sabs + 3 * F32 * s.abs()
    smax = s.abs().amax(dim=-1)
    dsm = ds.amax(dim=-1)
    tmax = s.reshape(*s.shape[:-1], 128, 32).amax(dim=-1)                                 # [n, 8, Tk, 128]
    grow = torch.zeros_like(tmax)
    grow[..., 1:] = (tmax[..., 1:] > torch.cummax(tmax, dim=-1)[0][..., :-1] - 2 * dsm[..., None]).double()
    ng = grow.sum(dim=-1)
    eps = dsm + F32 * (4 * smax + 2 + 3 * ng)                                             # [n, 8, Tk]
    e2 = torch.exp(2 * eps)[..., None]
    PX = torch.einsum("nhtj,njc->nhtc", P, Xa)
    V = torch.einsum("njc,hdc->nhjd", X, wv)                                              # [n, 8, T, 16]
    PV = P @ V
    devV = torch.sqrt((P @ (V * V) - PV * PV).clamp_(min=0.0))                            # [n, 8, Tk, 16]
    eX = _pair_err(Xa)
    pairs = torch.einsum("nhtj,njc->nhtc", P, eX) + torch.einsum("nhtj,njc->nhtc", PAIR * P + SUB / 4096.0, Xa + eX) \
        + torch.einsum("nhtj,njc->nhtc", H16 * P + SUB / 4096.0, _lo_abs(Xa))
    At = torch.einsum("nhtbj,nbjc->nhtbc", P.reshape(n, NH, Tk, 128, 32), Xa.reshape(n, 128, 32, C)).cumsum(dim=3)
    acc = F32 * (((6 + grow)[..., None] * At).sum(dim=3) + 16 * At[:, :, :, -1])
    eU = e2 * (pairs + acc + (10 + ng)[..., None] * F32 * PX)
    core = (e2 - 1) * devV + torch.einsum("nhtc,hdc->nhtd", eU, wva) + 257 * F32 * torch.einsum("nhtc,hdc->nhtd", U.abs() + eU, wva)
    return out, core + F32 * (out.abs() + core)


def _finish_t2i(o):
    """[n, 8, Tk, 16] -> [n, Tk, 128]"""
    return o.permute(0, 2, 1, 3).reshape(o.shape[0], o.shape[2], CI)


def t2i_ref_chunks(inp, chunk=2):
    """Yields (lo, hi, ref, bound), fp64 [hi - lo, Tk, 128], chunk by chunk of prompts."""
    B = inp["q"].shape[0]
    for lo in range(0, B, chunk):
        hi = min(lo + chunk, B)
        o, b = _t2i_chunk(inp, lo, hi, None)
        yield lo, hi, _finish_t2i(o), _finish_t2i(b)


def t2i_ref(inp, mutation=None, chunk=2):
    """``inp``: a dict of make_t2i (keys [B, 4096, 256], pos [4096, 256], q [B, Tk, 128], wk, wv [128, 256], bv [128] fp32, denom) ->
    (ref, bound) fp64 [B, Tk, 128]; with a mutation (ref, None)."""
    assert mutation is None or mutation in T2I_MUTATIONS, mutation
    if mutation is None:
        parts = list(t2i_ref_chunks(inp, chunk))
        return torch.cat([p[2] for p in parts]), torch.cat([p[3] for p in parts])
    B = inp["q"].shape[0]
    one = None if mutation in ("swap_heads", "prompt_from_next") else mutation
    ref = torch.cat([_finish_t2i(_t2i_chunk(inp, lo, min(lo + chunk, B), one)[0]) for lo in range(0, B, chunk)])
    if mutation == "swap_heads":                                                          # heads 0 and 1 land in each other's channels
        ref = torch.cat([ref[..., 16:32], ref[..., :16], ref[..., 32:]], dim=-1)
    if mutation == "prompt_from_next":
        ref = torch.roll(ref, -1, dims=0)
    return ref, None


def hadamard16():
    h = torch.ones(1, 1)
    for _ in range(4):
        h = torch.cat([torch.cat([h, h], dim=1), torch.cat([h, -h], dim=1)])
    return h


T2I_GENERATORS = ("diffuse", "needle", "rising", "flat", "plateau", "magnitudes", "distinct", "duel")
DUEL_ROWS = (5, 40)                                        # two keys of nearly equal weight, in the first and the second 32-key tile
NEEDLE_ROWS = (0, 31, 32, 4095, 63, 1, 33, 4094)          # token slot j -> the row of its dominant key: row 0, rows 31 | 32 (two LDS
#                                                           stages), the last row of all, the last row of the second stage, ...
PLATEAU_GAP = -math.log2(2048.99 / 4096.0) * math.log(2.0)  # score gap that puts 4096 p of every other key at 2048.99: fp16 keeps 2048


def make_t2i(name, B, Tk, seed=0):
    """Seeded operands of one msam_split16_t2i_attention call, on the CPU (fp32).  Wk = 0.25 [I_128 | 0] + noise / 512: the first 128
    stream channels (with pos) steer the scores, the last 128 carry the payload that the attention averages; except for diffuse and
    magnitudes (Wv ~ randn / 16) Wv = [0 | I_128] + noise / 1024, so an output channel shows one payload channel's error unaveraged.

    diffuse     the operands of tests/test_strict_host.py's t2i test with q x 1 (|s| up to ~15, a few dozen keys carry a row)
    needle      for every (prompt, head, token slot j) the key NEEDLE_ROWS[j] carries >= 0.999 of the weight (score 18, the rest noise)
    rising      the scores grow by 0.125 per 32-key tile along the stream (noise 0.04): the maximum grows in each of the 128 tiles
    flat        all scores equal (exactly 0: the steering channels of the stream and pos are zero, Wk has no noise)
    plateau     flat, but key 0 lies PLATEAU_GAP above the rest: every other key has 4096 p = 2048.99, whose fp16 value is 2048 - the
                lo halves of 4095 probabilities matter coherently, and all payload rows share a common part
    magnitudes  diffuse scores; the payload channels of the stream's rows scaled log-uniformly over 2^-12 .. 2^10
    distinct    every (prompt, head, token) prefers its own 128-key blocks (score 12) and the payload carries a +-1 pattern per block
    duel        per head ONE steering channel carries the score: the keys DUEL_ROWS hold 34 .. 35.5 there (fp16 spacing 2^-5, so the
                lo half of x + pos carries up to 4e-4 of the score of ~18), the query 8.3: two keys share the weight, their difference
                in score is the difference of two nearly equal large products - a score product that lost a cross term moves the
                weights by 1e-2 while the fp32 roundings move them by 1e-5"""
    assert name in T2I_GENERATORS and 1 <= Tk <= 8, (name, Tk)
    g = torch.Generator().manual_seed(1000 * seed + 31 * T2I_GENERATORS.index(name) + 7)

    def rn(*shape):
        return torch.randn(*shape, generator=g)

    keys, pos = rn(B, T, C), rn(T, C)
    wk, wv, bv = rn(CI, C) / 16, rn(CI, C) / 16, rn(CI) * 0.5
    q = rn(B, Tk, CI)
    codes = hadamard16()
    steer = torch.cat([0.25 * torch.eye(CI), torch.zeros(CI, C - CI)], dim=1)
    if name == "diffuse":
        keys = keys * torch.exp(0.3 * rn(B, T, 1))
    elif name == "magnitudes":
        wk[:, CI:] = 0.0                                                                  # the scaled channels stay out of the scores
        keys[:, :, CI:] = keys[:, :, CI:] * torch.exp2(torch.rand(B, T, 1, generator=g) * 22 - 12)
    else:
        exact = name in ("flat", "plateau", "duel")
        wk = steer + (0.0 if exact else 1.0) * rn(CI, C) / 512
        wk[:, CI:] = 0.0 if exact else wk[:, CI:]
        wv = torch.cat([torch.zeros(CI, C - CI), torch.eye(CI)], dim=1) + rn(CI, C) / 1024     # a value channel is (nearly) one payload channel
        keys[:, :, :CI] = 0.05 * keys[:, :, :CI]
        pos[:, :CI] = 0.0
        if name == "needle":
            q = torch.empty(B, Tk, NH, HD)
            for j in range(Tk):
                for h in range(NH):
                    code = codes[(j + 3 * h) % 16]
                    pos[NEEDLE_ROWS[j], h * HD:(h + 1) * HD] = 6.0 * code
                    q[:, j, h] = 3.0 * code
            q = q.reshape(B, Tk, CI) * (1.0 + 0.01 * rn(B, Tk, CI))
        elif name == "rising":
            dirs = torch.where(rn(NH, HD) > 0, 1.0, -1.0)
            pos[:, :CI] = (torch.arange(T).float()[:, None, None] / T * 5.333 * dirs).reshape(T, CI)
            q = (3.0 * dirs).reshape(1, 1, CI) * (1.0 + 0.01 * rn(B, Tk, CI))
        elif name in ("flat", "plateau"):
            keys[:, :, :CI] = 0.0
            if name == "plateau":
                dirs = torch.where(rn(NH, HD) > 0, 1.0, -1.0)
                q = dirs.reshape(1, 1, CI).expand(B, Tk, CI).clone()                      # s = q . (0.25 pos) / 4 = pos0 (exact powers of two)
                pos[0, :CI] = (PLATEAU_GAP * dirs).reshape(CI)
                keys[:, :, CI:] = 0.25 * keys[:, :, CI:] + rn(1, 1, C - CI)               # a common payload: the errors add up coherently
        elif name == "duel":
            a = 34.0 + torch.rand(NH, generator=g)
            pos[DUEL_ROWS[0], 0:CI:HD] = a
            pos[DUEL_ROWS[1], 0:CI:HD] = a + 0.3 * rn(NH)
            q = torch.zeros(B, Tk, NH, HD)
            q[..., 0] = 8.3 * (1.0 + 0.01 * rn(B, Tk, NH))
            q = q.reshape(B, Tk, CI)
        elif name == "distinct":
            blk = torch.arange(T) // 128
            pos[:, :CI] = (4.0 * codes[(blk[:, None] + torch.arange(NH)[None, :]) % 16]).reshape(T, CI)
            idx = (torch.arange(B)[:, None, None] * Tk + torch.arange(Tk)[None, :, None] + 3 * torch.arange(NH)[None, None, :]) % 16
            q = (3.0 * codes[idx]).reshape(B, Tk, CI) * (1.0 + 0.01 * rn(B, Tk, CI))
            keys[:, :, CI:] = 0.5 * keys[:, :, CI:] + torch.where(rn(32, C - CI) > 0, 1.0, -1.0)[blk]
    inp = {"keys": keys.float().contiguous(), "pos": pos.float().contiguous(), "q": q.float().contiguous(), "wk": wk.float().contiguous(),
           "wv": wv.float().contiguous(), "bv": bv.float(), "denom": 4.0}
    check_t2i_domain(inp)
    return inp


def check_t2i_domain(inp):
    """|x + pos| < 2^15, 64 |G| inside fp16's range, |score| log2 e <= 30."""
    xp = inp["keys"].double() + inp["pos"].double()
    assert xp.abs().max().item() < 2.0 ** 15
    G = torch.einsum("nthd,hdc->nhtc", _heads(inp["q"].double()), inp["wk"].double().reshape(NH, HD, C)) / inp["denom"]
    assert 64.0 * G.abs().max().item() < FP16_MAX
    smax = max(torch.einsum("jc,htc->htj", xp[p], G[p]).abs().max().item() for p in range(xp.shape[0]))
    assert smax * LOG2E <= 30.0, smax
    return smax


# ----------------------------------------------------------------------------------------------------------------------------- i2t
LN_EPS = 1e-5
I2T_FORMS = ("folded", "unfolded")


def _layernorm(r, w, b, eps):
    mu = r.mean(dim=-1, keepdim=True)
    dev = r - mu
    sig = torch.sqrt((dev * dev).mean(dim=-1, keepdim=True) + eps)
    return dev / sig * w + b, mu, dev, sig


def _ln_bound(r, E, y, mu, dev, sig, lw, lb):
    """The LayerNorm step of the module docstring: the pre-norm error E carried through two-pass fp32 statistics."""
    Ebar = E.mean(dim=-1, keepdim=True) + 260 * F32 * (r.abs() + E).mean(dim=-1, keepdim=True)
    E2 = torch.sqrt((E * E).mean(dim=-1, keepdim=True)) + 260 * F32 * (r.abs() + E).mean(dim=-1, keepdim=True) + 70 * F32 * sig
    den = sig - E2
    den = torch.where(den > 0, den, torch.zeros_like(den))                                # (never with these generators: bound = inf)
    yb = lw.abs() * ((E + Ebar) / den + dev.abs() * E2 / (sig * den)) + 8 * F32 * (r.abs() + mu.abs() + E) * lw.abs() / den \
        + 2 * F32 * lb.abs()
    return yb + F32 * (y.abs() + yb)


def _i2t_chunk(inp, lo, hi, forms, mutation):
    B, Tk = inp["tok_k"].shape[:2]
    n = hi - lo
    denom = float(inp["denom"])
    ws_q, ws_o = float(inp["wq_scale"]), float(inp["wo_scale"])
    if not inp["shared"]:
        X = inp["keys"][lo:hi].double()
    elif mutation == "shared_read_per_prompt":                                            # prompt p reads stream min(p, streams - 1)
        X = inp["keys"][torch.arange(lo, hi).clamp(max=inp["keys"].shape[0] - 1)].double()
    else:
        X = inp["keys"][0:1].double().expand(n, -1, -1)
    pos = inp["pos"].double()
    tok = (torch.arange(lo, hi) + 1) % B if mutation == "neighbour_tokens" else torch.arange(lo, hi)
    k = _heads(inp["tok_k"][tok].double())                                                # [n, Tk, 8, 16]
    v = _heads(inp["tok_v"][tok].double())
    wq = inp["wq"].double().reshape(NH, HD, C)
    wo = inp["wo"].double().reshape(C, NH, HD)
    bq = inp["bq"].double().reshape(NH, HD)
    bo, lw, lb = inp["bo"].double(), inp["ln_w"].double(), inp["ln_b"].double()
    xp = X + pos
    if mutation == "drop_lo":
        xp = hi16(xp)
    G = torch.einsum("nthd,hdc->nhtc", k, wq) / denom                                     # [n, 8, Tk, 256]
    beta = torch.einsum("nthd,hd->nht", k, bq) / denom                                    # [n, 8, Tk]
    s0 = torch.einsum("njc,nhtc->njht", xp, G)                                            # [n, T, 8, Tk]
    s = s0 + (0.0 if mutation == "no_beta" else beta[:, None])
    if mutation == "swap_heads":                                                          # heads 0 and 1 take each other's probabilities
        s = torch.cat([s[:, :, 1:2], s[:, :, 0:1], s[:, :, 2:]], dim=2)
    if mutation == "pad_unmasked":                                                        # 8 - Tk padding slots: score 0, value 0
        a = torch.softmax(torch.cat([s, s.new_zeros(*s.shape[:-1], 8 - Tk)], dim=-1), dim=-1)[..., :Tk]
    else:
        a = torch.softmax(s, dim=-1)
    if mutation == "drop_lo":
        a = hi16(a * 4096.0) / 4096.0
    VO = torch.einsum("chd,nthd->nhtc", wo, v)                                            # [n, 8, Tk, 256]
    att = a.reshape(n, T, NH * Tk) @ VO.reshape(n, NH * Tk, C)
    r = att + (0.0 if mutation == "no_bo" else bo) + (0.0 if mutation == "no_residual" else X)
    y, mu, dev, sig = _layernorm(r, lw, lb, float(inp["ln_eps"]))
    if mutation is not None:
        return y, None
    # ---- the bounds of the module docstring
    xpa, ka, va, wqa, woa = xp.abs(), k.abs(), v.abs(), wq.abs(), wo.abs()
    ex = (F32 + PAIR) * xpa + SUB
    smax = s.abs().amax(dim=-1)                                                           # [n, T, 8]
    VOa = torch.einsum("chd,nthd->nhtc", woa, va)
    sdev = []
    for h in range(NH):                                                                   # sqrt(a @ VO^2 - (a @ VO)^2), head by head
        ubar = a[:, :, h] @ VO[:, h]
        sdev.append(torch.sqrt((a[:, :, h] @ (VO[:, h] * VO[:, h]) - ubar * ubar).clamp_(min=0.0)))
    bounds = []
    for form in forms:
        if form == "folded":
            Ga = G.abs()
            eG = 17 * F32 * torch.einsum("nthd,hdc->nhtc", ka, wqa) / denom + _pair_err(Ga, 64.0)
            ebeta = 17 * F32 * torch.einsum("nthd,hd->nht", ka, bq.abs()) / denom
            rep = torch.einsum("njc,nhtc->njht", ex, Ga) + torch.einsum("njc,nhtc->njht", xpa + ex, eG)
            lolo = torch.einsum("njc,nhtc->njht", _lo_abs(xpa), _lo_abs(Ga, 64.0))
            sabs = torch.einsum("njc,nhtc->njht", xpa + ex, Ga + eG)
            ds = rep + lolo + (31 + 47.0 / 512) * F32 * sabs + 4 * F32 * (s0.abs() + beta.abs()[:, None]) + ebeta[:, None]
            eps = ds.amax(dim=-1) + F32 * (2 * smax + 2)                                  # [n, T, 8]
            e2 = torch.exp(2 * eps)
            eVO = 16 * F32 * VOa + _pair_err(VO.abs(), 64.0)
            E = torch.zeros_like(r)
            for h in range(NH):
                E += (e2[:, :, h, None] - 1) * sdev[h]
            W = (a * e2[..., None]).reshape(n, T, NH * Tk)
            Vr = (VO.abs() + eVO).reshape(n, NH * Tk, C)
            aV = W @ VO.abs().reshape(n, NH * Tk, C)
            E += 10 * F32 * aV + W @ eVO.reshape(n, NH * Tk, C) + PAIR * (W @ Vr) + (SUB / 4096.0) * Vr.sum(dim=1, keepdim=True)
            E += H16 * (W @ _lo_abs(VO.abs(), 64.0).reshape(n, NH * Tk, C)) \
                + (SUB / 4096.0) * _lo_abs(VO.abs(), 64.0).reshape(n, NH * Tk, C).sum(dim=1, keepdim=True)
            E += 27 * F32 * (1 + 2.0 ** -9) * (W @ Vr)
            E += 3 * F32 * (r.abs() + bo.abs() + E)
        else:
            # projection 1: K = 256, 8 k-tiles of 6 MFMAs; x iq + bq
            ew = _pair_err(wqa, ws_q)
            qa = torch.einsum("njc,hdc->njhd", xpa + ex, wqa + ew)
            eq = torch.einsum("njc,hdc->njhd", ex, wqa) + torch.einsum("njc,hdc->njhd", xpa + ex, ew) \
                + torch.einsum("njc,hdc->njhd", _lo_abs(xpa), _lo_abs(wqa, ws_q)) + (6 * 8 + 15) * F32 * (1 + 2.0 ** -9) * qa
            eq = eq + 2 * F32 * (qa + bq.abs())
            # scores: 8 fmaf per lane, the pair's sum, the product with the rounded 1 / denom x log2(e); one exponential
            ds = torch.einsum("njhd,nthd->njht", eq, ka) / denom + 11 * F32 * torch.einsum("njhd,nthd->njht", qa + bq.abs() + eq, ka) / denom
            eps = ds.amax(dim=-1) + F32 * (2 * smax + 2)
            e2 = torch.exp(2 * eps)
            # attention output per head channel: weights off by e^(2 eps), l (15 F), 1 / l, the product (F each), Tk fmaf
            vh = v.permute(0, 2, 1, 3)                                                    # [n, 8, Tk, 16]
            ah = a.permute(0, 2, 1, 3)                                                    # [n, 8, T, Tk]
            ao = ah @ vh                                                                  # [n, 8, T, 16]
            adev = torch.sqrt((ah @ (vh * vh) - ao * ao).clamp_(min=0.0))
            e2h = e2.permute(0, 2, 1)[..., None]                                          # [n, 8, T, 1]
            eatt = (e2h - 1) * adev + e2h * (17 + Tk) * F32 * (ah @ vh.abs())
            eatt = eatt.permute(0, 2, 1, 3).reshape(n, T, CI)                             # [n, T, 128]
            atta = ao.abs().permute(0, 2, 1, 3).reshape(n, T, CI)
            wo2 = woa.reshape(C, CI)
            ea = eatt + _pair_err(atta + eatt)
            ewo = _pair_err(wo2, ws_o)
            full = (atta + ea) @ (wo2 + ewo).t()
            E = ea @ wo2.t() + (atta + ea) @ ewo.t() + _lo_abs(atta + eatt) @ _lo_abs(wo2, ws_o).t() \
                + (6 * 4 + 15) * F32 * (1 + 2.0 ** -9) * full
            E = E + 3 * F32 * (r.abs() + bo.abs() + E)
        bounds.append(_ln_bound(r, E, y, mu, dev, sig, lw, lb))
    return y, bounds


def i2t_ref_chunks(inp, forms=I2T_FORMS, chunk=1):
    """Yields (lo, hi, ref, [bound of each form]), fp64 [hi - lo, 4096, 256], chunk by chunk of prompts."""
    B = inp["tok_k"].shape[0]
    for lo in range(0, B, chunk):
        hi = min(lo + chunk, B)
        y, bounds = _i2t_chunk(inp, lo, hi, tuple(forms), None)
        yield lo, hi, y, bounds


def i2t_ref(inp, form="folded", mutation=None, chunk=1):
    """``inp``: a dict of make_i2t -> (ref, bound of ``form``) fp64 [B, 4096, 256]; with a mutation (ref, None)."""
    assert form in I2T_FORMS and (mutation is None or mutation in I2T_MUTATIONS), (form, mutation)
    if mutation is None:
        parts = list(i2t_ref_chunks(inp, (form,), chunk))
        return torch.cat([p[2] for p in parts]), torch.cat([p[3][0] for p in parts])
    B = inp["tok_k"].shape[0]
    return torch.cat([_i2t_chunk(inp, lo, min(lo + chunk, B), (), mutation)[0] for lo in range(0, B, chunk)]), None


I2T_GENERATORS = ("diffuse", "flat", "magnitudes", "distinct", "duel")


def make_i2t(name, B, Tk, shared, seed=0):
    """Seeded operands of one image -> token block, on the CPU (fp32): keys [B (shared: 2), 4096, 256] - with a shared stream the kernel
    reads stream 0 only and stream 1 holds the NEGATED stream that it must not read -, pos, wq [128, 256], bq, tok_k / tok_v
    [B, Tk, 128], wo [256, 128], bo, ln_w, ln_b.

    diffuse     the operands of tests/test_strict_host.py's i2t test, bq of std 1 (the folded beta term carries weight)
    flat        tok_k = 0: all scores equal, so 8 - Tk padding slots taking part would take (8 - Tk) / 8 of the weight; the values of a
                prompt share a common part, so the attention term is large whatever the weights are
    magnitudes  Wq reads the first 128 stream channels only; the last 128 channels of the stream's rows are scaled log-uniformly over
                2^-12 .. 2^10
    distinct    diffuse, plus: tok_v of (prompt, head) carries 2 x a code vector of (prompt + head)
    duel        (Tk >= 2) Wq = 0.25 [I_128 | 0]; token 0 reads stream channel 16 h of head h, token 1 channel 16 h + 1 (tok_k 8.3 there,
                0 elsewhere), and pos holds 34 .. 35 in these two channels of every row: two scores of ~18 per row and head whose
                difference decides the weights, with up to 4e-4 of each score in the lo half of x + pos"""
    assert name in I2T_GENERATORS and 1 <= Tk <= 16, (name, Tk)
    g = torch.Generator().manual_seed(1000 * seed + 31 * I2T_GENERATORS.index(name) + 3)

    def rn(*shape):
        return torch.randn(*shape, generator=g)

    x, pos = rn(1 if shared else B, T, C), rn(T, C)
    wq, bq = rn(CI, C) / 16, rn(CI)
    wo, bo = rn(C, CI) / 11, rn(C) * 0.1
    lw, lb = torch.rand(C, generator=g) + 0.5, rn(C) * 0.2
    k, v = rn(B, Tk, CI), rn(B, Tk, CI)
    if name == "flat":
        k = torch.zeros_like(k)
        v = 0.5 * v + 1.5 * rn(B, 1, CI)
    elif name == "magnitudes":
        wq[:, CI:] = 0.0
        x[:, :, CI:] = x[:, :, CI:] * torch.exp2(torch.rand(x.shape[0], T, 1, generator=g) * 22 - 12)
    elif name == "duel":
        assert Tk >= 2
        wq = torch.cat([0.25 * torch.eye(CI), torch.zeros(CI, C - CI)], dim=1)
        x[:, :, :CI] = 0.05 * x[:, :, :CI]
        pos[:, :CI] = 0.0
        pos[:, 0:CI:HD] = 34.0 + torch.rand(T, NH, generator=g)
        pos[:, 1:CI:HD] = 34.0 + torch.rand(T, NH, generator=g)
        k = torch.zeros(B, Tk, NH, HD)
        k[:, 0, :, 0] = 8.3 * (1.0 + 0.01 * rn(B, NH))
        k[:, 1, :, 1] = 8.3 * (1.0 + 0.01 * rn(B, NH))
        k = k.reshape(B, Tk, CI)
        bq = bq * 0.1
    elif name == "distinct":
        codes = hadamard16()
        ph = (torch.arange(B)[:, None] + torch.arange(NH)[None, :]) % 16
        v = v + 2.0 * codes[ph][:, None].expand(B, Tk, NH, HD).reshape(B, Tk, CI)
    if shared:
        x = torch.cat([x, -x])
    inp = {"keys": x.float().contiguous(), "pos": pos.float().contiguous(), "wq": wq.float().contiguous(), "bq": bq.float(),
           "tok_k": k.float().contiguous(), "tok_v": v.float().contiguous(), "wo": wo.float().contiguous(), "bo": bo.float(),
           "ln_w": lw.float(), "ln_b": lb.float(), "ln_eps": LN_EPS, "denom": 4.0, "shared": bool(shared)}
    inp["wq_scale"], inp["wo_scale"] = weight_scale(inp["wq"]), weight_scale(inp["wo"])
    check_i2t_domain(inp)
    return inp


def check_i2t_domain(inp):
    """|x + pos| < 2^15, 64 |G| and 64 |VO| inside fp16's range, |score| log2 e <= 30."""
    B = inp["tok_k"].shape[0]
    k, v = _heads(inp["tok_k"].double()), _heads(inp["tok_v"].double())
    G = torch.einsum("nthd,hdc->nhtc", k, inp["wq"].double().reshape(NH, HD, C)) / inp["denom"]
    beta = torch.einsum("nthd,hd->nht", k, inp["bq"].double().reshape(NH, HD)) / inp["denom"]
    VO = torch.einsum("chd,nthd->nhtc", inp["wo"].double().reshape(C, NH, HD), v)
    assert 64.0 * G.abs().max().item() < FP16_MAX and 64.0 * VO.abs().max().item() < FP16_MAX
    smax = 0.0
    for p in range(B):
        xp = inp["keys"][0 if inp["shared"] else p].double() + inp["pos"].double()
        assert xp.abs().max().item() < 2.0 ** 15
        smax = max(smax, (torch.einsum("jc,htc->jht", xp, G[p]) + beta[p]).abs().max().item())
    assert smax * LOG2E <= 30.0, smax
    return smax


# ----------------------------------------------------------------------------------------------------------------------------- up2
# THE up2 BOUND (``up2_ref``; msam_strict_upscale2 = s16_up2_kernel).  Row = (prompt, token, first sub-pixel s1), 64 channels:
#   z1 = LayerNorm2d(u1 row), h1 = GELU(z1), z2 = h1 W2^T + b2 (128 = (second sub-pixel s2, 32 channels)), h2 = GELU(z2),
#   low[p][m][4 ty + 2 ky + ky2][4 tx + 2 kx + kx2] = hyper[p][mask0 + m] . h2[s2 = 2 ky2 + kx2]
# * LayerNorm, two-pass fp32 statistics over the lane pair's 64 channels: the mean is a chain of <= 18 additions and one exchange:
#   dmu = 20 F mean |x|; d = x - mean: F |d| + dmu; the sum of squares (the same chain over d^2) and + eps, sqrtf, the division:
#   16 F relative on rstd; d rstd w + b: 3 F |z1 - b| + F |z1|.
# * gelu_p8(x) = max(x, 0) - t 2^q(t), t = min(|x|, 9), q a degree-8 polynomial for log2(erfc(t / sqrt 2) / 2): the reference is the
#   erf GELU, so the polynomial's own approximation error counts, evaluated here in fp64 element by element (|gelu_p8 in fp64 - erf
#   form|); the fp32 evaluation adds: Horner, 8 FMAs: 9 F Q(t) with Q the chain on absolute values (an error of q is a relative error
#   ln 2 dq of 2^q), v_exp_f32 2 F, the product and the subtraction 2 F; slope <= 1.13 for what arrives from upstream.
# * the product, K = 64: h1 (scale 1) and W2 (w_scale) as pairs, 4 k-steps x 3 MFMAs on one accumulator: 27 roundings; x 1 / w_scale
#   + b2: 2 F.
# * the hyper product: per lane 8 packed multiply-adds (2 F each, contracted or not), the two halves' sum and the exchange: 18 F
#   |hyper| . |h2| on top of |hyper| . e_h2.
UP2_MUTATIONS = ("mask0_ignored", "unshuffle_swapped", "second_gelu_missing", "hyper_ld_ignored", "drop_lo")
UP2_GENERATORS = ("diffuse", "magnitudes")
_P8 = (-1.6902803281482193e-06, 2.5081630155909806e-05, -0.00011445332347648218, -0.000323369400575757, 0.0073334285989403725,
       -0.05271423980593681, -0.4591154158115387, -1.151123285293579, -0.9999988675117493)


def _p8(t, absolute=False):
    q = torch.full_like(t, abs(float(torch.tensor(_P8[0], dtype=torch.float32))) if absolute else float(torch.tensor(_P8[0], dtype=torch.float32)))
    for c in _P8[1:]:
        c = float(torch.tensor(c, dtype=torch.float32))                                   # the coefficients as the kernel holds them
        q = q * t + (abs(c) if absolute else c)
    return q


def _gelu_erf(z):
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def _gelu_p8_err(z, ez):
    """Error of the kernel's GELU against the erf form for an argument z known to ez."""
    t = z.abs().clamp(max=9.0)
    tail = t * torch.exp2(_p8(t))
    approx = (torch.relu(z) - tail - _gelu_erf(z)).abs()
    own = tail * (math.log(2.0) * 9 * F32 * _p8(t, absolute=True) + 2 * F32) + 2 * F32 * (torch.relu(z) + tail)
    return GELU_SLOPE * ez + approx + own


def _up2_chunk(inp, p, mutation):
    dev = inp["u1"].device
    x = inp["u1"][p * 16384:(p + 1) * 16384].double()                                     # [16384, 64]
    lw, lb, eps = inp["ln_w"].double(), inp["ln_b"].double(), float(inp["ln_eps"])
    w2, b2, s = inp["w2"].double(), inp["b2"].double(), float(inp["w_scale"])
    mask0, nmask, ld = int(inp["mask0"]), int(inp["nmask"]), int(inp["hyper_ld"])
    hyp = inp["hyper"].double()                                                           # [P, 4, ld]
    if mutation == "hyper_ld_ignored":
        hyp = hyp.reshape(-1)[:hyp.shape[0] * 4 * 32].reshape(hyp.shape[0], 4, 32) if ld == 32 else \
            torch.stack([hyp.reshape(-1)[(q * 4 + m) * 32:(q * 4 + m) * 32 + 32] for q in range(hyp.shape[0]) for m in range(4)]).reshape(-1, 4, 32)
    hy = hyp[p, :nmask, :32] if mutation == "mask0_ignored" else hyp[p, mask0:mask0 + nmask, :32]
    mu = x.mean(dim=-1, keepdim=True)
    d = x - mu
    sig = torch.sqrt((d * d).mean(dim=-1, keepdim=True) + eps)
    z1 = d / sig * lw + lb
    h1 = _gelu_erf(z1)
    w2m = w2
    if mutation == "drop_lo":
        h1, w2m = hi16(h1), hi16(w2 * s) / s
    z2 = h1 @ w2m.t() + b2
    h2 = z2 if mutation == "second_gelu_missing" else _gelu_erf(z2)                       # [16384, 128]

    def unshuffle(m):                                                                     # [16384 (ty, tx, ky, kx), nmask, 4 (ky2, kx2)] -> [nmask, 256, 256]
        t = m.reshape(64, 64, 2, 2, nmask, 2, 2)                                          # ty, tx, ky, kx, m, ky2, kx2
        if mutation == "unshuffle_swapped":
            t = t.transpose(5, 6)
        return t.permute(4, 0, 2, 5, 1, 3, 6).reshape(nmask, 256, 256)

    out = unshuffle(torch.einsum("mc,rsc->rms", hy, h2.reshape(16384, 4, 32)))
    if mutation is not None:
        return out, None
    dmu = 20 * F32 * x.abs().mean(dim=-1, keepdim=True)
    ed = F32 * d.abs() + dmu
    ez1 = lw.abs() * (ed / sig + 16 * F32 * d.abs() / sig) + 3 * F32 * (z1 - lb).abs() + F32 * z1.abs()
    eh1 = _gelu_p8_err(z1, ez1)
    h1a, w2a = h1.abs(), w2.abs()
    ea = eh1 + _pair_err(h1a + eh1)
    ew = _pair_err(w2a, s)
    full = (h1a + ea) @ (w2a + ew).t()
    ez2 = ea @ w2a.t() + (h1a + ea) @ ew.t() + _lo_abs(h1a + eh1) @ _lo_abs(w2a, s).t() + 27 * F32 * (1 + 2.0 ** -9) * full
    ez2 = ez2 + 2 * F32 * (z2.abs() + b2.abs() + ez2)
    eh2 = _gelu_p8_err(z2, ez2)
    bound = torch.einsum("mc,rsc->rms", hy.abs(), (eh2 + 18 * F32 * (h2.abs() + eh2)).reshape(16384, 4, 32))
    return out, unshuffle(bound)


def up2_ref_chunks(inp):
    """Yields (p, ref, bound), fp64 [nmask, 256, 256], prompt by prompt."""
    for p in range(int(inp["P"])):
        yield (p,) + _up2_chunk(inp, p, None)


def up2_ref(inp, mutation=None):
    assert mutation is None or mutation in UP2_MUTATIONS, mutation
    parts = [_up2_chunk(inp, p, mutation) for p in range(int(inp["P"]))]
    return torch.stack([a for a, _ in parts]), (None if mutation is not None else torch.stack([b for _, b in parts]))


def make_up2(name, P, mask0, nmask, hyper_ld, seed=0):
    """Seeded operands of one msam_strict_upscale2 call, on the CPU (fp32): u1 [P * 16384, 64], ln_w, ln_b [64], w2 [128, 64], b2 [128],
    hyper [P, 4, hyper_ld] (the columns from 32 on hold values the kernel must not read).
    diffuse: the operands of tests/test_strict_host.py's up2 test; magnitudes: the rows of u1 scaled log-uniformly over 2^-12 .. 2^10."""
    assert name in UP2_GENERATORS and hyper_ld >= 32 and 0 <= mask0 and nmask >= 1 and mask0 + nmask <= 4
    g = torch.Generator().manual_seed(1000 * seed + 31 * UP2_GENERATORS.index(name) + 11)

    def rn(*shape):
        return torch.randn(*shape, generator=g)

    u1 = rn(P * 16384, 64)
    if name == "diffuse":
        u1 = u1 * torch.exp(0.5 * rn(P * 16384, 1))
    else:
        u1 = u1 * torch.exp2(torch.rand(P * 16384, 1, generator=g) * 22 - 12)
    inp = {"u1": u1.contiguous(), "ln_w": torch.rand(64, generator=g) + 0.5, "ln_b": rn(64) * 0.2, "ln_eps": 1e-6,
           "w2": (rn(128, 64) / 8).contiguous(), "b2": rn(128) * 0.1, "hyper": (rn(P, 4, hyper_ld) + 3.0 * torch.arange(4).float()[None, :, None]).contiguous(),
           "hyper_ld": hyper_ld, "mask0": mask0, "nmask": nmask, "P": P}
    inp["w_scale"] = weight_scale(inp["w2"])
    assert inp["u1"].abs().max().item() < 2.0 ** 15 and inp["w2"].abs().max().item() * inp["w_scale"] < FP16_MAX
    return inp


# -------------------------------------------------------------------------------------------------------------------------- relpos
# THE relpos BOUND (``relpos_ref``; msam_split16_relpos_attention = srelpos_mfma_kernel<HD, true> for the 64 x 64 grid, window 0, and
# srelpos_win_mfma_kernel<HD, true> for the 14 x 14 windows of the zero-padded grid, whose padded tokens are the qkv bias and DO take
# part as keys, as upstream's zero padding after norm1 makes them).  S = 64 or 14, HD = 64 or 80, HH = HD / 2, NKS = HH / 8:
#   score = (scale q) . k + q . R_h[qh - kh + S - 1] + q . R_w[qw - kw + S - 1],  softmax over the S^2 keys,  out = P @ v
# * qs = q x fl(scale log2 e): the rounded constants and the product, 3 F |qs|, then the pair; k as a pair.  NKS k-steps x 3 MFMAs on
#   one accumulator: REP + LOLO + (16 + 3 NKS - 1) F Sabs.  The row term: HH fmaf per lane half, the exchange, x log2 e: (HH + 3) F
#   |q| . |R_h|; the column term: HH f32-input MFMA steps of 2 products, x log2 e: (2 HH + 2) F |q| . |R_w|; the two additions: 2 F |s|.
# * exponentials in the log domain: the own one F (2 smax + 2), and per later 32-key tile (nt = S^2 / 32 rounded up) the rescale's
#   exponential and product, 3 F, their arguments telescoping to 2 smax: eps = max_k ds + F (4 smax + 2 + 3 (nt - 1)).
# * l is a plain running sum in key order, 16 additions per tile and lane and one rescale, magnitude-aware: the sum after tile t is
#   L_t (in units of the final sum): 17 F sum_t L_t, + the exchange and the division 3 F; relative, on |out| <= P @ |v|.
# * P @ v: the exponentials as pairs of 4096 p, v as pairs; per tile 6 MFMAs and one rescale on an accumulator: F (7 sum_t A_t + 16
#   A_last) with A_t the part of P @ |v| from the tiles <= t.
RELPOS_MUTATIONS = ("rel_h_w_swapped", "padded_keys_unmasked", "no_qkv_bias", "crossed_heads", "drop_lo")
RELPOS_GENERATORS = ("diffuse", "needle", "distinct")


def _rel_index(S, dev):
    i = torch.arange(S, device=dev)
    return i[:, None] - i[None, :] + S - 1                                                # [q, k]


def relpos_ref(inp, mutation=None):
    """``inp``: a dict of make_relpos -> (ref, bound) fp64 [B G G, heads HD]; with a mutation (ref, None)."""
    assert mutation is None or mutation in RELPOS_MUTATIONS, mutation
    B, heads, hd, G, window, scale = (inp[k] for k in ("B", "heads", "hd", "G", "window", "scale"))
    dev = inp["qkv"].device
    D = heads * hd
    S = window if window else G
    x = inp["qkv"].double().reshape(B, G, G, 3 * D)
    nW = (G + S - 1) // S
    pad = nW * S - G
    if pad:
        x = torch.nn.functional.pad(x, (0, 0, 0, pad, 0, pad))
        fill = torch.zeros_like(inp["bqkv"].double()) if mutation == "no_qkv_bias" else inp["bqkv"].double()
        x[:, G:, :, :] = fill
        x[:, :, G:, :] = fill
    x = x.reshape(B, nW, S, nW, S, 3, heads, hd).permute(5, 0, 1, 3, 6, 2, 4, 7).reshape(3, B * nW * nW, heads, S * S, hd)
    q, k, v = x.unbind(0)                                                                 # [Bp, heads, S^2, hd]
    if mutation == "crossed_heads" and heads > 1:
        k = torch.roll(k, 1, dims=1)
    rh, rw = inp["rel_h"].double(), inp["rel_w"].double()
    if mutation == "rel_h_w_swapped":
        rh, rw = rw, rh
    idx = _rel_index(S, dev)
    NKS, HH, nt = hd // 16, hd // 2, (S * S + 31) // 32
    outs, bounds = [], []
    for h in range(heads):                                                                # head by head: the scores are [Bp, S^2, S^2]
        qh_, kh_, vh_ = q[:, h], k[:, h], v[:, h]
        if mutation == "drop_lo":
            kh_, vh_ = hi16(kh_), hi16(vh_)
        qg = qh_.reshape(-1, S, S, hd)
        bh = torch.einsum("bhwc,hkc->bhwk", qg, rh[idx])                                  # [Bp, qh, qw, kh]
        bw = torch.einsum("bhwc,wkc->bhwk", qg, rw[idx])
        sqk = scale * (qh_ @ kh_.transpose(-1, -2))
        s = (sqk.reshape(-1, S, S, S, S) + bh[..., :, None] + bw[..., None, :]).reshape(-1, S * S, S * S)
        if mutation == "padded_keys_unmasked":                                            # the keys S^2 .. 32 nt - 1 of the last tile: score 0, value 0
            P = torch.softmax(torch.cat([s, s.new_zeros(*s.shape[:-1], 32 * nt - S * S)], dim=-1), dim=-1)[..., :S * S]
        else:
            P = torch.softmax(s, dim=-1)
        if mutation == "drop_lo":
            p = torch.exp(s - s.amax(dim=-1, keepdim=True))
            P = hi16(p * 4096.0) / 4096.0 / p.sum(dim=-1, keepdim=True)
        o = P @ vh_
        outs.append(o)
        if mutation is not None:
            continue
        qsa, ka, va = (scale * qh_).abs(), kh_.abs(), vh_.abs()
        eq = 3 * F32 * qsa + _pair_err(qsa)
        ek = _pair_err(ka)
        sabs = (qsa + eq) @ (ka + ek).transpose(-1, -2)
        ds = eq @ ka.transpose(-1, -2) + (qsa + eq) @ ek.transpose(-1, -2) + _lo_abs(qsa) @ _lo_abs(ka).transpose(-1, -2) \
            + (16 + 3 * NKS - 1) * F32 * sabs + 2 * F32 * s.abs()
        qa = qg.abs()
        ebh = (HH + 3) * F32 * torch.einsum("bhwc,hkc->bhwk", qa, rh[idx].abs())
        ebw = (2 * HH + 2) * F32 * torch.einsum("bhwc,wkc->bhwk", qa, rw[idx].abs())
        ds = (ds.reshape(-1, S, S, S, S) + ebh[..., :, None] + ebw[..., None, :]).reshape(-1, S * S, S * S)
        smax = s.abs().amax(dim=-1)
        assert float(smax.max()) * LOG2E <= 30.0 and float(qsa.max()) * LOG2E < FP16_MAX, "outside the documented domain"
        eps = ds.amax(dim=-1) + F32 * (4 * smax + 2 + 3 * (nt - 1))                       # [Bp, S^2]
        e2 = torch.exp(2 * eps)[..., None]
        dev_v = torch.sqrt((P @ (vh_ * vh_) - o * o).clamp_(min=0.0))
        padk = 32 * nt - S * S
        Pt = torch.nn.functional.pad(P, (0, padk)).reshape(*P.shape[:-1], nt, 32)
        Vt = torch.nn.functional.pad(va, (0, 0, 0, padk)).reshape(va.shape[0], nt, 32, hd)
        At = torch.einsum("bqtj,btjc->bqtc", Pt, Vt).cumsum(dim=2)
        acc = F32 * (7 * At.sum(dim=2) + 16 * At[:, :, -1])
        Lt = Pt.sum(dim=-1).cumsum(dim=-1)
        lrel = F32 * (17 * Lt.sum(dim=-1, keepdim=True) + 3)
        ev = _pair_err(va)
        pairs = P @ ev + (PAIR * P + SUB / 4096.0) @ (va + ev) + (H16 * P + SUB / 4096.0) @ _lo_abs(va)
        PV = P @ va
        core = (e2 - 1) * dev_v + e2 * (pairs + acc + lrel * PV)
        bounds.append(core + F32 * (o.abs() + core))

    def back(parts):                                                                      # [heads][Bp, S^2, hd] -> [B G G, heads hd]
        t = torch.stack(parts, dim=1).reshape(B, nW, nW, heads, S, S, hd).permute(0, 1, 4, 2, 5, 3, 6).reshape(B, nW * S, nW * S, D)
        return t[:, :G, :G].reshape(B * G * G, D)

    return back(outs), (None if mutation is not None else back(bounds))


def make_relpos(name, B, heads, hd, G, window, seed=0):
    """Seeded operands of one msam_split16_relpos_attention call, on the CPU (fp32): qkv [B G G, 3 heads hd], bqkv, rel_h / rel_w
    [2 S - 1, hd].
    diffuse   the operands of tests/test_strict_host.py's relpos test
    needle    every query carries a common +-1 pattern u and the k part of the qkv BIAS is 1.25 u: the padded keys of a border
              window (the last window rows and columns of a grid that is no multiple of 14) carry the weight, the output is the v
              bias; on an exact grid key 0 of every (window or global) sequence takes that role
    distinct  diffuse, plus a +-2 pattern per (image, head) in v and a pattern per head in k"""
    assert name in RELPOS_GENERATORS
    g = torch.Generator().manual_seed(1000 * seed + 31 * RELPOS_GENERATORS.index(name) + 13 + G + hd)

    def rn(*shape):
        return torch.randn(*shape, generator=g)

    D = heads * hd
    S = window if window else G
    qkv = rn(B, G, G, 3, heads, hd)
    bqkv = rn(3, heads, hd) * 0.5
    rel_h, rel_w = rn(2 * S - 1, hd) * 0.2, rn(2 * S - 1, hd) * 0.2
    if name == "needle":
        u = torch.where(rn(hd) > 0, 1.0, -1.0)                                            # score of the needle: sqrt(hd) x 1.0 x 1.25 = 10 / 11.2
        qkv[:, :, :, 0] = 0.5 * qkv[:, :, :, 0] + u
        rel_h, rel_w = 0.5 * rel_h, 0.5 * rel_w
        needle = 1.25 * u * (1.0 + 0.01 * rn(heads, hd))
        bqkv[1] = needle
        if G % S == 0:
            qkv[:, ::S, ::S, 1] = needle
    elif name == "distinct":
        codes = torch.where(rn(B * heads, hd) > 0, 2.0, -2.0).reshape(B, 1, 1, heads, hd)
        qkv[:, :, :, 2] = qkv[:, :, :, 2] + codes
        qkv[:, :, :, 1] = qkv[:, :, :, 1] + 0.5 * torch.where(rn(heads, hd) > 0, 1.0, -1.0)
    inp = {"qkv": qkv.reshape(B * G * G, 3 * D).float().contiguous(), "bqkv": bqkv.reshape(3 * D).float().contiguous(),
           "rel_h": rel_h.float().contiguous(), "rel_w": rel_w.float().contiguous(), "B": B, "heads": heads, "hd": hd, "G": G,
           "window": window, "scale": hd ** -0.5}
    return inp                                                                            # (relpos_ref asserts the domain: it has the scores)



def widen_t2i(inp, B):
    """``inp`` (a few prompts, on any device) -> B prompts without drawing B streams on the CPU: prompt p takes stream p % n rolled by
    p // n rows and the tokens of prompt p % n with their channels rolled by 16 (p // n) (one head further): every prompt differs from
    every other, and the scores keep their distribution."""
    n = inp["q"].shape[0]
    keys = torch.stack([torch.roll(inp["keys"][p % n], p // n, dims=0) for p in range(B)])
    q = torch.stack([torch.roll(inp["q"][p % n], 16 * (p // n), dims=-1) for p in range(B)])
    return dict(inp, keys=keys.contiguous(), q=q.contiguous())


def widen_i2t(inp, B):
    """The same for make_i2t operands with a SHARED stream: B prompts' tokens from those of a few."""
    assert inp["shared"]
    n = inp["tok_k"].shape[0]
    k = torch.stack([torch.roll(inp["tok_k"][p % n], 16 * (p // n), dims=-1) for p in range(B)])
    v = torch.stack([torch.roll(inp["tok_v"][p % n], 16 * (p // n), dims=-1) * (1.0 + 0.01 * (p // n)) for p in range(B)])
    return dict(inp, tok_k=k.contiguous(), tok_v=v.contiguous())
