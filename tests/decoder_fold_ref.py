"""fp64 references, elementwise error bounds, input generators, mutated references and a rounded restatement for the two folded
attention kernels of the mask decoder: msam_t2i_fold_attention (csrc/decfold.hip: fold_q_kernel, fold_attn_kernel, fold_finish_kernel)
and msam_i2t_fold_layer (variant 1: fold_frag_kernel + i2t_tok_kernel of csrc/decfold_tok.hip; variant 0: fold_q_kernel, fold_v_kernel,
fold_i2t_kernel of csrc/decfold.hip).  A plain module: no fixtures, no kernel calls.  Everything is torch and follows the device of its
operands; the references work in chunks of prompts.

The operations, on the VALUES of the 16-bit operands, in the UNFOLDED formulation of the reference model (so the folding is under test).
T = 4096 image tokens, 8 heads of 16 channels, scale 1/4; h is a head, d one of its 16 channels, c one of the 256 stream channels:

  t2i   K = keys Wk^T + tabk,  V = keys Wv^T + bv,   out[p, t, 16 h + d] = sum_j P_j V[j, 16 h + d],
        P = softmax_j(s),  s_j = q[p, t, h] . K[j, h] / 4                                                           -> [P, Nt, 128]
  i2t   q = x Wq^T + tabq,  a[j, h, :] = softmax over the Nt prompt tokens of  q[j, h] . k[p, t, h] / 4,
        r_j = x_j + sum_h Wo[:, h] (sum_t a[j, h, t] v[p, t, h]) + bo,   y_j = LayerNorm_256(r_j; ln_w, ln_b, eps)     -> [P, 4096, 256]

tabk / tabq are inputs in the 16-bit type: their rounding is not a kernel error.  u = 2^-8 (bf16) / 2^-11 (fp16) is the unit roundoff of
the operands' type, SUB = 2^-25 the absolute rounding error below fp16's normal range (0 for bf16), F = 2^-24 the unit roundoff of fp32.

THE t2i BOUND (``t2i_ref``), term by term from the rounding points of the kernels:

  * fold_q_kernel rounds Q'[h, t] = Wk_h^T q[h, t] (256 channels, 16 fp32 FMAs each) to 16 bit:
        errQ_c = u |Q'_c| + (1 + u) 16 F sum_d |q_d| |Wk[d, c]| + SUB.
    It perturbs the SCORES: |ds_j| <= |keys_j| . errQ / 4.  The score is 9 chained MFMA steps of 32 products, each step summed in an
    unspecified order and scaled by 0.25 (exact): a product passes <= 32 roundings in its step and one per later step, 43 F of
    Sabs_j = (|keys_j| . (|Q'| + errQ) + |tabk_j| . |q|) / 4.  Every exp() (argument a <= 0) has a log error <= F (2 |a| + 2): the
    subtraction, the log2(e) product and the 1-ulp v_exp_f32.  A key's weight passes its own exp (|a| <= 2 smax), the rescales
    alpha = exp(m_old - m_new) of the later tiles (the |a| telescope to <= 2 smax; <= 128 results) and the merge's exp(m_i - M)
    (|a| <= 2 smax): F (12 smax + 260) in all.  With
        eps = max_j |keys_j| . errQ / 4 + 43 F max_j Sabs_j + F (12 smax + 260)
    the kernel's weights are P'_j = P_j e^(d_j) / sum_k P_k e^(d_k), |d| <= eps, so |P'_j - P_j| <= (e^(2 eps) - 1) P_j and, because
    sum_j (P'_j - P_j) = 0,   |sum_j P'_j V_j - out| = |sum_j (P'_j - P_j)(V_j - out)| <= (e^(2 eps) - 1) (P @ |V - out|).
    No first-order step: this holds for any eps.
  * the un-normalised probabilities are rounded to 16 bit before the second MFMA while l sums the unrounded ones.  The value
    projection is linear and acts on the normalised 256-channel vector, so a relative error d_j of p_j reaches the output as
    sum_j P'_j d_j (keys_j . Wv_d):  u e^(2 eps) (P @ |Z|), Z = V - bv; probabilities below fp16's normal range: SUB sum_j |Z_j| (l >= 1).
  * fp32 accumulation, all relative to G = |Wv| (P @ |keys|) >= P @ |Z|: O' (128 chained steps of 32 products, each step followed by a
    rescale: 2 * 128 + 32 = 288 F), l (the same chain, 8 in-lane adds, 2 cross-lane steps, the merge: 314 F), the merge of the splits
    and the 256-term projection chain (256 + 16 + 16 = 288 F): 890 F e^(2 eps) G.  For KS = 1 the normalised vector enters the
    projection MFMA as a 16-bit hi + lo pair: u^2 G more (+ SUB sum_c |Wv_dc| for lo below fp16's normal range).
  * the output is rounded once: u |got| (+ SUB), and |got| <= |out| + everything above; the bias add: 2 F |bv|.

THE i2t BOUNDS (``i2t_ref(variant=...)``).  Pre-norm row r, its error E_c elementwise:

  * K'[h, t] = Wq_h^T k[h, t] rounded to 16 bit (fold_q_kernel; fold_frag_kernel after a product with 0.25 log2(e): 2 more roundings,
    18 F for both): errK as errQ above.  Variant 1 ALSO rounds the table operand 0.25 log2(e) k to 16 bit (variant 0 multiplies the
    exact k and scales by 0.25 afterwards): (u |tabq_j| . |k| + SUB sum |tabq_j|) / 4 more.  43 F Sabs for the fp32 score, F (6 smax + 6)
    for the one exp and the rounded constant.  eps[j, h] = max_t of the sum; as above, the attention part of r moves by at most
        sum_h (e^(2 eps[j, h]) - 1) sum_t a_t |U_t - ubar|,   U[h, t] = Wo[:, h] v[h, t],  ubar = sum_t a_t U_t,
    and sum_t a_t |U_t - ubar| <= sqrt(sum_t a_t U_t^2 - ubar^2) (Jensen; a matrix product instead of a [T, 8, Nt, 256] tensor).
  * the NORMALISED probabilities (rcp: 1 ulp) are rounded to 16 bit: (u + 4 F) per probability; SUB below fp16's normal range.
  * V'[h, t] is rounded to 16 bit: variant 0 V' = U, bo enters the accumulator in fp32; variant 1 V' = U + bo / 8 (t < Nt), so that
    the rounded probabilities of a head, which need not sum to 1, also scale bo / 8.  errU = u |V'| + (1 + u) 18 F (|Wo| |v| + |bo| / 8)
    + SUB, weighted by the kernel's probabilities <= (1 + u) e^(2 eps) a.
  * fp32 accumulation of r (three MFMA steps over 64 + 32 products): 100 F (|x| + |bo| + sum p |V'|).
  * the error of r is carried through the LayerNorm without linearising.  With mu, dev = r - mu, sig = sqrt(var + ln_eps), and
    Ebar = mean_c E, E2 = rms_c E:  |mu' - mu| <= Ebar, |dev' - dev| <= E + Ebar, |sig' - sig| <= E2 (centring is a projection, and
    x -> sqrt(x^2 + ln_eps) is 1-Lipschitz), so
        |y' - y| <= |ln_w| ((E + Ebar) / (sig - E2) + |dev| E2 / (sig (sig - E2))),
    the slope |ln_w| / sig and the mean / variance terms.  The kernels' one-pass fp32 statistics add 270 F mean|r| to Ebar and
    540 F mean(r^2) / sig to E2 (sum of squares minus squared mean), the two FMAs and rsqrt 8 F (|r| + |mu|) |ln_w| / (sig - E2) + 2 F |ln_b|.
  * the output is rounded once: u |got| + SUB.

The generators keep |s| below 60 and sig of order 1 (tests/test_decoder_fold_ref_host.py checks it): the fp32 terms stay small
against u, and sig - E2 stays positive.  ``restate_t2i`` / ``restate_i2t`` redo the FOLDED arithmetic in fp64 with a 16-bit rounding at
exactly the rounding points above (everything fp32 in the kernels stays fp64): they must lie within one bound of the reference, which
keeps the bound honest from below.  T2I_MUTATIONS / I2T_MUTATIONS name the defects these kernels are prone to as variants of the
references; the host test proves each at least 4 bounds from the truth on the generator meant for it."""
import math

import torch

T, H, HD, C, CI = 4096, 8, 16, 256, 128
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
SUB = {torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}
F32 = 2.0 ** -24
LN_EPS = 1e-5

T2I_MUTATIONS = ("drop_last_tile", "drop_split", "merge_no_rescale", "no_tabk", "no_bv", "swap_heads", "prompt_from_next",
                 "swap_v_rows")
I2T_MUTATIONS = ("pad_unmasked", "no_bo", "bo_over_nt", "no_residual", "no_tabq", "swap_heads", "neighbour_tokens",
                 "shared_reads_own_stream", "last_tile_unchanged")
SWAP_V = (T - 1, T - 2)                      # the two keys whose value rows "swap_v_rows" exchanges


def key_splits(P):
    """KS of csrc/decfold.hip, the smallest power of two with P * KS >= 512, at most 16: 16 for P <= 63, 8 for 64..127, 4 for 128..255,
    2 for 256..511, 1 from 512."""
    ks = 1
    while P * ks < 512 and ks < 16:
        ks *= 2
    return ks


def round16(t, dtype):
    return t.to(dtype).double()


def _heads(t):
    """[..., 128] -> [..., 8, 16]"""
    return t.reshape(*t.shape[:-1], H, HD)


# ------------------------------------------------------------------------------------------------------------------------- t2i
def _t2i_chunk(inp, lo, hi, mutation, ks):
    dtype = inp["qtok"].dtype
    u, sub = U[dtype], SUB[dtype]
    q = _heads(inp["qtok"][lo:hi].double()).permute(0, 2, 1, 3)                          # [n, 8, Nt, 16]
    X = (inp["keys"][0:1] if inp["kv_shared"] else inp["keys"][lo:hi]).double()          # [1 | n, T, 256]
    wk, wv = inp["wk"].double().reshape(H, HD, C), inp["wv"].double().reshape(H, HD, C)
    tab = _heads(inp["tabk"].double()).permute(1, 0, 2)                                  # [8, T, 16]
    bv = inp["bv"].double().reshape(H, 1, HD)
    if mutation == "no_tabk":
        tab = torch.zeros_like(tab)
    if mutation == "no_bv":
        bv = torch.zeros_like(bv)
    K = torch.einsum("bjc,hdc->bhjd", X, wk) + tab                                       # [1 | n, 8, T, 16]
    Z = torch.einsum("bjc,hdc->bhjd", X, wv)
    V = Z + bv
    if mutation == "swap_v_rows":
        V = V.clone()
        V[:, :, list(SWAP_V)] = V[:, :, list(SWAP_V[::-1])]
    s = q @ K.transpose(-1, -2) / 4.0                                                    # [n, 8, Nt, T]
    sm = s
    if mutation == "drop_last_tile":
        sm = s.clone()
        sm[..., T - 32:] = -math.inf
    elif mutation == "drop_split":                                                       # the split that starts at key T / 2
        assert ks > 1
        sm = s.clone()
        sm[..., T // 2:T // 2 + T // ks] = -math.inf
    elif mutation == "merge_no_rescale":                                                 # every split relative to its OWN maximum
        assert ks > 1
        sp = s.reshape(*s.shape[:-1], ks, T // ks)
        sm = (sp - sp.amax(dim=-1, keepdim=True)).reshape(s.shape)
    P = torch.softmax(sm, dim=-1)
    out = P @ V                                                                          # [n, 8, Nt, 16]
    if mutation is not None:
        return out, None
    # ---- the bound of the module docstring
    Qp = torch.einsum("nhtd,hdc->nhtc", q, wk)
    errQ = u * Qp.abs() + (1 + u) * 16 * F32 * torch.einsum("nhtd,hdc->nhtc", q.abs(), wk.abs()) + sub
    Xa = X.abs().expand(q.shape[0], -1, -1)
    dq = torch.einsum("njc,nhtc->nhtj", Xa, errQ).amax(dim=-1) / 4.0
    sabs = (torch.einsum("njc,nhtc->nhtj", Xa, Qp.abs() + errQ) + q.abs() @ tab.abs().transpose(-1, -2)).amax(dim=-1) / 4.0
    smax = s.abs().amax(dim=-1)
    eps = dq + 43 * F32 * sabs + F32 * (12 * smax + 260)                                 # [n, 8, Nt]
    e2 = torch.exp(2 * eps)[..., None]
    A = torch.stack([(P[:, :, t] [..., None, :] @ (V - out[:, :, t, None, :]).abs())[..., 0, :] for t in range(q.shape[2])], dim=2)
    Bz = P @ Z.abs()
    G = torch.einsum("nhtc,hdc->nhtd", torch.einsum("nhtj,njc->nhtc", P, Xa), wv.abs())
    core = (e2 - 1) * A + e2 * (u * Bz + 890 * F32 * G) + u * u * G + 2 * F32 * bv.abs()
    core = core + sub * (Z.abs().sum(dim=2)[:, :, None, :] + wv.abs().sum(dim=-1)[None, :, None, :])
    return out, core + u * (out.abs() + core) + sub


def _finish_t2i(o):
    """[n, 8, Nt, 16] -> [n, Nt, 128]"""
    return o.permute(0, 2, 1, 3).reshape(o.shape[0], o.shape[2], CI)


def t2i_ref_chunks(inp, chunk=8):
    """Yields (lo, hi, ref, bound), fp64 [hi - lo, Nt, 128], chunk by chunk of prompts."""
    Pn = inp["qtok"].shape[0]
    for lo in range(0, Pn, chunk):
        hi = min(lo + chunk, Pn)
        o, b = _t2i_chunk(inp, lo, hi, None, key_splits(Pn))
        yield lo, hi, _finish_t2i(o), _finish_t2i(b)


def t2i_ref(inp, mutation=None, chunk=8):
    """``inp``: a dict of make_t2i (keys [Pk, 4096, 256], qtok [P, Nt, 128], wk, wv [128, 256], tabk [4096, 128] 16 bit, bv fp32 [128],
    kv_shared) -> (ref, bound) fp64 [P, Nt, 128]; with a mutation (ref, None)."""
    assert mutation is None or mutation in T2I_MUTATIONS, mutation
    if mutation is None:
        parts = list(t2i_ref_chunks(inp, chunk))
        return torch.cat([p[2] for p in parts]), torch.cat([p[3] for p in parts])
    Pn = inp["qtok"].shape[0]
    one = None if mutation in ("swap_heads", "prompt_from_next") else mutation
    ref = torch.cat([_finish_t2i(_t2i_chunk(inp, lo, min(lo + chunk, Pn), one, key_splits(Pn))[0]) for lo in range(0, Pn, chunk)])
    if mutation == "swap_heads":                                                         # heads 0 and 1 land in each other's channels
        ref = torch.cat([ref[..., 16:32], ref[..., :16], ref[..., 32:]], dim=-1)
    if mutation == "prompt_from_next":
        ref = torch.roll(ref, -1, dims=0)
    return ref, None


def restate_t2i(inp, chunk=8):
    """The folded arithmetic of fold_q_kernel / fold_attn_kernel / fold_finish_kernel in fp64 with the kernels' 16-bit roundings: Q'
    rounded; per key split an online softmax over 32-key tiles whose probabilities (relative to the RUNNING maximum) are rounded before
    they multiply the stream tile while l sums the unrounded ones; the (m, l, O') partials merged; the value projection applied to the
    normalised 256-channel vector; one output rounding.  (The hi + lo pair of the KS = 1 epilogue carries the vector to u^2 and is kept
    exact here.)"""
    dtype = inp["qtok"].dtype
    Pn, Nt = inp["qtok"].shape[:2]
    ks = key_splits(Pn)
    wk, wv = inp["wk"].double().reshape(H, HD, C), inp["wv"].double().reshape(H, HD, C)
    tab = _heads(inp["tabk"].double()).permute(1, 0, 2)
    outs = []
    for lo in range(0, Pn, chunk):
        q = _heads(inp["qtok"][lo:lo + chunk].double()).permute(0, 2, 1, 3)
        n = q.shape[0]
        X = (inp["keys"][0:1] if inp["kv_shared"] else inp["keys"][lo:lo + chunk]).double().expand(n, -1, -1)
        Qp = round16(torch.einsum("nhtd,hdc->nhtc", q, wk), dtype)
        s = (torch.einsum("njc,nhtc->nhtj", X, Qp) + q @ tab.transpose(-1, -2)) * 0.25
        Ms, Ls, Os = [], [], []
        for k in range(ks):
            m = torch.full((n, H, Nt), -1.0e30, dtype=torch.float64, device=s.device)
            l = torch.zeros_like(m)
            O = torch.zeros(n, H, Nt, C, dtype=torch.float64, device=s.device)
            for j0 in range(k * (T // ks), (k + 1) * (T // ks), 32):
                st = s[..., j0:j0 + 32]
                mn = torch.maximum(m, st.amax(dim=-1))
                alpha = torch.exp(m - mn)
                p = torch.exp(st - mn[..., None])
                l = l * alpha + p.sum(dim=-1)
                O = O * alpha[..., None] + torch.einsum("nhtj,njc->nhtc", round16(p, dtype), X[:, j0:j0 + 32])
                m = mn
            Ms.append(m), Ls.append(l), Os.append(O)
        M = torch.stack(Ms).amax(dim=0)
        sc = [torch.exp(m - M) for m in Ms]
        ll = sum(e * l for e, l in zip(sc, Ls))
        ctx = sum((e / ll)[..., None] * O for e, O in zip(sc, Os))
        o = torch.einsum("nhtc,hdc->nhtd", ctx, wv) + inp["bv"].double().reshape(H, 1, HD)
        outs.append(_finish_t2i(round16(o, dtype)))
    return torch.cat(outs)


# ------------------------------------------------------------------------------------------------------------------------- i2t
def _layernorm(r, w, b):
    mu = r.mean(dim=-1, keepdim=True)
    dev = r - mu
    sig = torch.sqrt((dev * dev).mean(dim=-1, keepdim=True) + LN_EPS)
    return dev / sig * w + b, mu, dev, sig


def _i2t_chunk(inp, lo, hi, variants, mutation):
    dtype = inp["ktok"].dtype
    u, sub = U[dtype], SUB[dtype]
    Pn, Nt = inp["ktok"].shape[:2]
    n = hi - lo
    src = slice(lo, hi)
    if not inp["x_shared"]:
        X = inp["x"][src].double()
    elif mutation == "shared_reads_own_stream":                                          # prompt p > 0 reads stream min(p, Px - 1)
        X = inp["x"][torch.arange(lo, hi).clamp(max=inp["x"].shape[0] - 1)].double()
    else:
        X = inp["x"][0:1].double()
    tok = (torch.arange(lo, hi) + 1) % Pn if mutation == "neighbour_tokens" else torch.arange(lo, hi)
    k = _heads(inp["ktok"][tok].double())                                                # [n, Nt, 8, 16]
    v = _heads(inp["vtok"][tok].double())
    wq = inp["wq"].double().reshape(H, HD, C)
    wo = inp["wo"].double().reshape(C, H, HD)
    tab = _heads(inp["tabq"].double())                                                   # [T, 8, 16]
    bo, lw, lb = inp["bo"].double(), inp["ln_w"].double(), inp["ln_b"].double()
    if mutation == "no_tabq":
        tab = torch.zeros_like(tab)
    qh = torch.einsum("bjc,hdc->bjhd", X, wq) + tab                                      # [1 | n, T, 8, 16]
    s = torch.einsum("njhd,nthd->njht", qh.expand(n, -1, -1, -1), k) / 4.0               # [n, T, 8, Nt]
    Uv = torch.einsum("chd,nthd->nhtc", wo, v)                                           # [n, 8, Nt, 256]
    if mutation == "swap_heads":                                                         # heads 0 and 1 take each other's probabilities
        s = torch.cat([s[:, :, 1:2], s[:, :, 0:1], s[:, :, 2:]], dim=2)
    if mutation == "pad_unmasked":                                                       # 8 - Nt padding tokens: score 0, value 0
        a = torch.softmax(torch.cat([s, s.new_zeros(*s.shape[:-1], 8 - Nt)], dim=-1), dim=-1)[..., :Nt]
    else:
        a = torch.softmax(s, dim=-1)
    att = a.reshape(n, T, H * Nt) @ Uv.reshape(n, H * Nt, C)
    bias = {"no_bo": 0.0, "bo_over_nt": 8.0 / Nt}.get(mutation, 1.0) * bo
    r = att + bias + (0.0 if mutation == "no_residual" else X)
    y, mu, dev, sig = _layernorm(r, lw, lb)
    if mutation == "last_tile_unchanged":
        y = y.clone()
        y[:, T - 16:] = X[:, T - 16:]
    if mutation is not None:
        return y, None
    # ---- the bounds of the module docstring
    Xa = X.abs().expand(n, -1, -1)
    Kp = torch.einsum("nthd,hdc->nhtc", k, wq)
    errK = u * Kp.abs() + (1 + u) * 18 * F32 * torch.einsum("nthd,hdc->nhtc", k.abs(), wq.abs()) + sub
    dscore0 = torch.einsum("njc,nhtc->njht", Xa, errK) / 4.0
    tabk_abs = torch.einsum("jhd,nthd->njht", tab.abs(), k.abs()) / 4.0
    sabs = torch.einsum("njc,nhtc->njht", Xa, Kp.abs() + errK) / 4.0 + tabk_abs
    smax = s.abs().amax(dim=-1)
    sdev = []
    for h in range(H):                                                                   # sqrt(sum_t a_t U_t^2 - ubar^2), head by head
        ubar = a[:, :, h] @ Uv[:, h]
        sdev.append(torch.sqrt((a[:, :, h] @ (Uv[:, h] * Uv[:, h]) - ubar * ubar).clamp_(min=0.0)))
    Uabs0 = torch.einsum("chd,nthd->nhtc", wo.abs(), v.abs())
    bounds = []
    for variant in variants:
        dscore = dscore0
        if variant == 1:
            dscore = dscore0 + u * tabk_abs + sub * tab.abs().sum(dim=-1)[None, :, :, None] / 4.0
        eps = (dscore + 43 * F32 * sabs).amax(dim=-1) + F32 * (6 * smax + 6)             # [n, T, 8]
        e2 = torch.exp(2 * eps)
        Vp = Uv + bo / 8.0 if variant == 1 else Uv
        Uabs = Uabs0 + (bo.abs() / 8.0 if variant == 1 else 0.0)
        errU = u * Vp.abs() + (1 + u) * 18 * F32 * Uabs + sub
        E = torch.zeros_like(r)
        for h in range(H):                                                               # score perturbation (Jensen)
            E += (e2[:, :, h, None] - 1) * sdev[h]
        W = (a * e2[..., None]).reshape(n, T, H * Nt)                                    # >= the kernel's probabilities / (1 + u)
        Vr = (Vp.abs() + errU).reshape(n, H * Nt, C)
        pv = W @ Vr
        E += (u + 4 * F32) * pv + (1 + u) * (W @ errU.reshape(n, H * Nt, C)) + sub * Vr.sum(dim=1, keepdim=True)
        E += 100 * F32 * ((1 + u) * pv + Xa + (bo.abs() if variant == 0 else 0.0))
        Ebar = E.mean(dim=-1, keepdim=True) + 270 * F32 * (r.abs() + E).mean(dim=-1, keepdim=True)
        E2 = torch.sqrt((E * E).mean(dim=-1, keepdim=True)) + 540 * F32 * ((r.abs() + E) ** 2).mean(dim=-1, keepdim=True) / sig
        den = sig - E2
        den = torch.where(den > 0, den, torch.zeros_like(den))                           # (never with these generators: bound = inf)
        yb = lw.abs() * ((E + Ebar) / den + dev.abs() * E2 / (sig * den)) + 8 * F32 * (r.abs() + mu.abs() + E) * lw.abs() / den \
            + 2 * F32 * lb.abs()
        bounds.append(yb + u * (y.abs() + yb) + sub)
    return y, bounds


def i2t_ref_chunks(inp, variants=(1, 0), chunk=4):
    """Yields (lo, hi, ref, [bound of each variant]), fp64 [hi - lo, 4096, 256], chunk by chunk of prompts."""
    Pn = inp["ktok"].shape[0]
    for lo in range(0, Pn, chunk):
        hi = min(lo + chunk, Pn)
        y, bounds = _i2t_chunk(inp, lo, hi, tuple(variants), None)
        yield lo, hi, y, bounds


def i2t_ref(inp, variant=1, mutation=None, chunk=4):
    """``inp``: a dict of make_i2t (x [Px, 4096, 256], ktok, vtok [P, Nt, 128], wq [128, 256], tabq [4096, 128], wo [256, 128] 16 bit,
    bo, ln_w, ln_b fp32, x_shared) -> (ref, bound of ``variant``) fp64 [P, 4096, 256]; with a mutation (ref, None)."""
    assert variant in (0, 1) and (mutation is None or mutation in I2T_MUTATIONS), (variant, mutation)
    if mutation is None:
        parts = list(i2t_ref_chunks(inp, (variant,), chunk))
        return torch.cat([p[2] for p in parts]), torch.cat([p[3][0] for p in parts])
    Pn = inp["ktok"].shape[0]
    return torch.cat([_i2t_chunk(inp, lo, min(lo + chunk, Pn), (), mutation)[0] for lo in range(0, Pn, chunk)]), None


def restate_i2t(inp, variant, chunk=4):
    """The folded arithmetic of the image->token layer in fp64 with the kernels' 16-bit roundings.  Variant 0: K' and V' rounded, the
    table term on the exact k, scores scaled by 0.25, normalised probabilities rounded, bo added in the accumulator.  Variant 1: K' and
    the table operand rounded AFTER the product with 0.25 log2(e), softmax through exp2, V' = U + bo / 8 rounded.  One output rounding."""
    dtype = inp["ktok"].dtype
    Pn, Nt = inp["ktok"].shape[:2]
    wq, wo = inp["wq"].double().reshape(H, HD, C), inp["wo"].double().reshape(C, H, HD)
    tab = _heads(inp["tabq"].double())
    bo, lw, lb = inp["bo"].double(), inp["ln_w"].double(), inp["ln_b"].double()
    scale = float(torch.tensor(0.25 * 1.4426950408889634, dtype=torch.float32))
    outs = []
    for lo in range(0, Pn, chunk):
        k, v = _heads(inp["ktok"][lo:lo + chunk].double()), _heads(inp["vtok"][lo:lo + chunk].double())
        n = k.shape[0]
        X = (inp["x"][0:1] if inp["x_shared"] else inp["x"][lo:lo + chunk]).double().expand(n, -1, -1)
        Kp = torch.einsum("nthd,hdc->nhtc", k, wq)
        Uv = torch.einsum("chd,nthd->nhtc", wo, v)
        if variant == 1:
            Kp, kt = round16(Kp * scale, dtype), round16(k * scale, dtype)
            s = torch.einsum("njc,nhtc->njht", X, Kp) + torch.einsum("jhd,nthd->njht", tab, kt)
            a = torch.exp2(s - s.amax(dim=-1, keepdim=True))
            Vp = round16(Uv + bo / 8.0, dtype)
        else:
            s = (torch.einsum("njc,nhtc->njht", X, round16(Kp, dtype)) + torch.einsum("jhd,nthd->njht", tab, k)) * 0.25
            a = torch.exp(s - s.amax(dim=-1, keepdim=True))
            Vp = round16(Uv, dtype)
        a = round16(a / a.sum(dim=-1, keepdim=True), dtype)
        r = a.reshape(n, T, H * Nt) @ Vp.reshape(n, H * Nt, C) + X + (bo if variant == 0 else 0.0)
        outs.append(round16(_layernorm(r, lw, lb)[0], dtype))
    return torch.cat(outs)


# --------------------------------------------------------------------------------------------------------------------- generators
T2I_GENERATORS = ("diffuse", "needle", "split_skew", "distinct")
I2T_GENERATORS = ("diffuse", "short", "distinct", "table")


def _codes():
    """32 code vectors of 16 channels: the rows of the 16 x 16 Hadamard matrix and their negatives (dot products 16, 0 or -16)."""
    h = torch.ones(1, 1)
    for _ in range(4):
        h = torch.cat([torch.cat([h, h], dim=1), torch.cat([h, -h], dim=1)])
    return torch.cat([h, -h])


def needle_tiles(ks):
    """First keys of the 32-key tiles that carry the needles: the last tile of all (keys 4064..4095), the last tile of the key split
    that ends at T / 2 and the first tile of the next one, and from KS = 4 the same pair at the end of the first split."""
    tiles = [T - 32, T // 2 - 32, T // 2]
    if ks >= 4:
        tiles += [T // ks - 32, T // ks]
    return tiles


def needle_key(code, head, ks):
    """Key of code vector ``code`` (0..31) for ``head``: 32 distinct keys per head, spread over needle_tiles(ks); (0, 0) -> key 4095."""
    tiles = needle_tiles(ks)
    return tiles[code % len(tiles)] + (31 - 3 * (code // len(tiles)) - head) % 32


def needle_code(p, t, head, Nt):
    return (5 * (p * Nt + t) + 11 * head) % 32


def make_t2i(name, dtype, P, Nt, shared, seed=0):
    """Seeded operands of one msam_t2i_fold_attention call, on the CPU.

    diffuse     the operands of tests/test_gpu_kernels.py::test_t2i_fold_attention (|s| up to ~30, a few dozen keys carry a row)
    needle      for every (prompt, head, token) ONE key carries >= 0.9999 of the weight: the query is 2 x a +-1 code vector and tabk
                of that key, for that head, 4 x the same code (score 32; the other code keys of the head score 0 or -32, the stream
                term is noise of std ~1).  The keys lie in needle_tiles(KS): the last tile of a key split, the first tile of the
                next, and keys 4064..4095; (prompt 0, token 0, head 0) sits on key 4095.  The output is V of that key within the
                bound, so a dropped tile or split, a wrong key -> value mapping or a crossed prompt / head is a wrong row
    split_skew  tabk adds 2.5 x (j // 256) x the sign of the row to the scores: the maxima of the key splits differ by 2.5 .. 37.5,
                ascending for even (prompt + token), descending for odd ones, and the stream carries a +-1 pattern per 256-key block so
                that the splits' own averages differ by construction
    distinct    diffuse, plus: every (prompt, head) prefers its own 128-key block (code vectors again, score +9) and the stream carries
                a +-1 pattern per block: prompts and heads differ by construction, not only by noise"""
    assert name in T2I_GENERATORS and dtype in U, (name, dtype)
    ks = key_splits(P)
    g = torch.Generator().manual_seed(1000 * seed + 31 * T2I_GENERATORS.index(name) + 7)

    def rn(*shape):
        return torch.randn(*shape, generator=g)

    Pk = 1 if shared else P
    keys, pe = rn(Pk, T, C), rn(T, C)
    wk, wv = rn(CI, C) / 16, rn(CI, C) / 16
    bk, bv = rn(CI), rn(CI)
    q = rn(P, Nt, CI) * 1.5
    tab = pe @ wk.to(dtype).float().t() + bk
    codes = _codes()
    block = torch.where(rn(32, C) > 0, 1.0, -1.0)                                        # +-1 pattern of a 128-key block
    if name == "needle":
        tab = rn(T, CI) * 0.1
        q = torch.empty(P, Nt, H, HD)
        for h in range(H):
            for c in range(32):
                tab[needle_key(c, h, ks), h * HD:(h + 1) * HD] = 4.0 * codes[c]
            idx = torch.tensor([[needle_code(p, t, h, Nt) for t in range(Nt)] for p in range(P)])
            q[:, :, h] = 2.0 * codes[idx]
        q = q.reshape(P, Nt, CI)
        keys = keys * 0.5
    elif name == "split_skew":
        wdir = torch.where(rn(H, HD) > 0, 0.25, -0.25)                                   # |w|^2 = 1 per head
        gj = 2.5 * (torch.arange(T) // 256).float()
        tab = rn(T, CI) * 0.1 + (gj[:, None, None] * wdir).reshape(T, CI)
        sign = 1.0 - 2.0 * ((torch.arange(P)[:, None] + torch.arange(Nt)[None, :]) % 2).float()
        q = rn(P, Nt, CI) * 0.5 + (4.0 * sign[:, :, None, None] * wdir).reshape(P, Nt, CI)
        keys = keys * 0.25 + block[torch.arange(T) // 256]
    elif name == "distinct":
        tab = tab + 0.75 * codes[(torch.arange(T) // 128) % 32].repeat(1, H)
        ph = (torch.arange(P)[:, None] + 3 * torch.arange(H)[None, :]) % 32              # [P, 8] -> preferred block
        q = q + 3.0 * codes[ph][:, None].expand(P, Nt, H, HD).reshape(P, Nt, CI)
        keys = keys * 0.5 + block[torch.arange(T) // 128]
    return {"keys": keys.to(dtype).contiguous(), "qtok": q.to(dtype).contiguous(), "wk": wk.to(dtype), "wv": wv.to(dtype),
            "tabk": tab.to(dtype).contiguous(), "bv": bv.float(), "kv_shared": bool(shared)}


def make_i2t(name, dtype, P, Nt, shared, seed=0):
    """Seeded operands of one msam_i2t_fold_layer call, on the CPU.

    diffuse     the operands of tests/test_gpu_kernels.py::test_i2t_fold_layer
    short       scores of order 1 (k x 0.5): the softmax over the Nt < 8 prompt tokens is nearly uniform, so 8 - Nt padding tokens
                taking part would take (8 - Nt) / 8 of the weight, and a bias shared as bo / Nt instead of bo / 8 is 8 / Nt of bo.  The
                values of a prompt share a common part (v = 1.5 c_p + 0.5 noise): the attention term is large whatever the weights
                are, so weight lost to padding shows, while the weights' own rounding moves it little
    table       the table term carries the scores: Wq x 0.25 and tabq of std 1.5, so a kernel without it is far off while the
                rounding of K' moves the scores little
    distinct    diffuse, plus: v of (prompt, head) carries 2 x code vector (prompt + head) % 32, and with a shared stream x holds a
                SECOND stream (the negated first) that the kernel must not read"""
    assert name in I2T_GENERATORS and dtype in U, (name, dtype)
    g = torch.Generator().manual_seed(1000 * seed + 31 * I2T_GENERATORS.index(name) + 3)

    def rn(*shape):
        return torch.randn(*shape, generator=g)

    Px = 1 if shared else P
    x, pe = rn(Px, T, C), rn(T, C)
    wq, bq = rn(CI, C) / 16, rn(CI)
    wo, bo = rn(C, CI) / math.sqrt(CI), rn(C)
    lw, lb = rn(C) * 0.2 + 1, rn(C)
    k, v = rn(P, Nt, CI), rn(P, Nt, CI)
    tabq = None
    if name == "short":
        k = k * 0.5
        v = 0.5 * v + 1.5 * rn(P, 1, CI)
    elif name == "table":
        wq = wq * 0.25
        tabq = rn(T, CI) * 1.5
    elif name == "distinct":
        codes = _codes()
        ph = (torch.arange(P)[:, None] + torch.arange(H)[None, :]) % 32
        v = v + 2.0 * codes[ph][:, None].expand(P, Nt, H, HD).reshape(P, Nt, CI)
        if shared:
            x = torch.cat([x, -x])
    if tabq is None:
        tabq = pe @ wq.to(dtype).float().t() + bq
    return {"x": x.to(dtype).contiguous(), "ktok": k.to(dtype).contiguous(), "vtok": v.to(dtype).contiguous(), "wq": wq.to(dtype),
            "tabq": tabq.to(dtype).contiguous(), "wo": wo.to(dtype), "bo": bo.float(), "ln_w": lw.float(), "ln_b": lb.float(),
            "x_shared": bool(shared)}


def to_device(inp, dev):
    return {n: (t.to(dev) if torch.is_tensor(t) else t) for n, t in inp.items()}
